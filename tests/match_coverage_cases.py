"""The cases the tests of scene coverage and selection of match records share (include/fdcm.h, "Match lists: scene coverage and
selection").  Not collected: the tests import it.

Record lists of about 60 records on the worlds of test_gpu_coverage.py (through select_cases.world): integer translations,
rotations by arbitrary float angles with non-integer M2 and M5, a non-uniform scale, posed lines within a pixel of the map's
sides (inside and outside), NaN and infinity in M, tmpl_idx below and above the set, the template without lines, the 300-line
template (more than one LDS chunk of 256 segments), exact duplicates, a cluster of near-duplicates, a window clipped to one
column and one clipped to nothing, and a tmpl_index_base other than 0.  The referee's coverage of a list is computed once per
(world, radius, bin_tolerance, margin) and shared."""
import functools

import numpy as np

import match_coverage_ref as MC
import match_ref as MR
import select_cases as SC
import select_ref as SR

f32 = np.float32
WORLDS = ("96x80-b0-d30", "96x80-b5-d6", "70x37-b5-d30", "70x37-b5-d30-bytes")
BASES = {"96x80-b0-d30": 0, "96x80-b5-d6": 7, "70x37-b5-d30": -3, "70x37-b5-d30-bytes": 0}


class MatchCase:
    """A world of select_cases (labels, frame, templates) with a record list."""

    def __init__(self, world, recs, base=0):
        self.w = world
        self.labels, self.keys, self.m = world.labels, world.keys, world.m
        self.border, self.width, self.height, self.W, self.H = world.border, world.width, world.height, world.W, world.H
        self.tmpls = world.tmpls
        self.T = (world.border, world.border)
        self.recs = np.ascontiguousarray(recs, dtype=MR.MATCH_DTYPE)
        self.base = base
        self._cov = {}

    def coverage(self, recs=None, labels=None, radius=2, bin_tolerance=1, margin=None):
        own = recs is None and labels is None
        key = (radius, bin_tolerance, margin)
        if own and key in self._cov:
            return self._cov[key]
        out = MC.coverage(self.labels if labels is None else labels, self.keys, self.T, self.W, self.H, self.tmpls,
                          self.recs if recs is None else recs, self.base, radius=radius, bin_tolerance=bin_tolerance, margin=margin)
        if own:
            self._cov[key] = out
        return out

    def select(self, radius=2, bin_tolerance=1, margin=None, **kw):
        counts, _, masks = self.coverage(radius=radius, bin_tolerance=bin_tolerance, margin=margin)
        return SR.rule(self.labels, counts, masks, **kw)

    def with_records(self, recs):
        return MatchCase(self.w, recs, self.base)


def placed(tm, width, height, border, rng, angle=0.0, sx=1.0, sy=1.0, at=None):
    """The float64 matrix of the lines tm (4, N) rotated by angle and scaled by (sx, sy) whose posed box lies inside the map at a
    random non-integer place, or with its lower corner at `at` (label coordinates)."""
    c, s = np.cos(angle), np.sin(angle)
    A = np.array([[c * sx, -s * sy], [s * sx, c * sy]])
    pts = np.concatenate([tm[:2], tm[2:]], axis=1).astype(np.float64) if tm.shape[1] else np.zeros((2, 1))
    q = A @ pts
    lo = np.array([-border + 0.25 - q[0].min(), -border + 0.25 - q[1].min()])
    hi = np.array([width + border - 1.25 - q[0].max(), height + border - 1.25 - q[1].max()])
    t = lo + rng.random(2) * np.maximum(hi - lo, 0.0) if at is None else np.asarray(at, dtype=np.float64) - [q[0].min(), q[1].min()]
    return [A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1]]


def record_list(world, base=0, seed=23):
    rng = np.random.default_rng(seed)
    width, height, border, tm = world.width, world.height, world.border, world.tmpls
    rows = []   # (tmpl, matrix)

    def add(t, M):
        rows.append((t, [float(v) for v in M]))
    for p in world.poses[:12]:                                                  # integer translations (some not admissible)
        add(int(p[0]), [1, 0, int(p[2]), 0, 1, int(p[3])])
    for t in (1, 2, 3, 5, 2, 3, 1, 5, 3, 2, 6, 3):                              # arbitrary angles, non-integer M2 and M5
        add(t, placed(tm[t], width, height, border, rng, angle=rng.uniform(-np.pi, np.pi) if t != 6 else 0.0))
    add(3, placed(tm[3], width, height, border, rng, angle=0.4, sx=1.3, sy=0.6))  # a non-uniform scale
    one = tm[1]                                                                 # the one-line template at the map's sides
    ex, ey = float(max(one[0, 0], one[2, 0]) - min(one[0, 0], one[2, 0])), float(max(one[1, 0], one[3, 0]) - min(one[1, 0], one[3, 0]))
    add(1, placed(one, width, height, border, rng, at=(-border - 0.75, 3.0)))                    # inside by a quarter pixel
    add(1, placed(one, width, height, border, rng, at=(3.0, -border - 0.5)))
    add(1, placed(one, width, height, border, rng, at=(width + border - 0.25 - ex, 3.0)))
    add(1, placed(one, width, height, border, rng, at=(3.0, height + border - 0.5 - ey)))
    add(1, placed(one, width, height, border, rng, at=(-border - 1.0, 3.0)))                     # outside: an end point at -1
    add(1, placed(one, width, height, border, rng, at=(3.0, height + border - ey)))              # outside: an end point at H
    add(1, placed(one, width, height, border, rng, at=(width + border - ex + 0.5, 3.0)))
    bad = placed(tm[2], width, height, border, rng, angle=0.3)
    add(2, bad[:2] + [np.nan] + bad[3:])                                        # NaN and infinity in M
    add(2, [np.inf] + bad[1:])
    add(3, bad[:4] + [-np.inf] + bad[5:])
    add(0, [1, 0, 5.5, 0, 1, 5.25])                                             # the template without lines
    add(4, placed(tm[4], width, height, border, rng, angle=0.0))                # 300 lines: two LDS chunks
    add(4, placed(tm[4], width, height, border, rng, angle=2.1))
    # template 7 is vertical at x = 3.25: a window a pixel wide
    far = 1.0 if border else -0.75
    add(7, [1, 0, width + far - 3.25 + 0.25, 0, 1, 2.0])                        # at margin 2 clipped to the last column (border > 0)
    add(7, [1, 0, width + (3.0 if border else -0.5) - 3.25 + 0.25, 0, 1, 2.5])  # at margin 2 clipped to nothing (border > 0)
    add(7, [1, 0, 10.5, 0, 1, 1.0])
    cl = placed(tm[3], width, height, border, rng, angle=0.7)                   # a cluster of near-duplicates
    for da, dx, dy in [(0, 0, 0), (0.01, 0.3, 0), (-0.01, 0, 0.4), (0.02, -0.6, 0.2), (0, 1.0, 1.0), (0.05, 2.0, -1.0)]:
        c, s = np.cos(0.7 + da), np.sin(0.7 + da)
        add(3, [c, -s, cl[2] + dx, s, c, cl[5] + dy])
    n0 = len(rows)
    dup = (12, 14, 26, 12, n0 - 6)                                              # exact duplicates, the score included
    rows += [rows[k] for k in dup]
    recs = MR.records([t + base for t, _ in rows], rng.uniform(0, 40, len(rows)), [M for _, M in rows])
    recs[n0:] = recs[list(dup)]
    bad_idx = MR.records([base - 1, base + len(tm), base + len(tm) + 1000, -(1 << 31)], [1, 2, 3, 4], [[1, 0, 5, 0, 1, 5]] * 4)
    return np.concatenate([recs[:20], bad_idx[:2], recs[20:], bad_idx[2:]])    # tmpl_idx below and above the set


@functools.lru_cache(maxsize=None)
def case(name):
    world = SC.world(name, False)
    return MatchCase(world, record_list(world, BASES[name]), BASES[name])


@functools.lru_cache(maxsize=None)
def pose_case(name):
    """The world's own pose list as records {1, 0, x, 0, 1, y}: identity 1."""
    world = SC.world(name, False)
    return MatchCase(world, MC.translation_records(world.poses))


@functools.lru_cache(maxsize=None)
def long_case():
    """select_cases.long_list as 270 one-line records on its 5-pixel lattice."""
    world = SC.long_list()
    return MatchCase(world, MC.translation_records(world.poses))


def check_identities(case, got, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024,
                     coverage=None):
    """Scene selection's identities on a result (selected, counts, residual) for the case's list; coverage: how to take the
    coverage of a sub-list (recs -> (counts, residual)), the referee's by default."""
    sel, counts, residual = got
    labels = case.labels
    assert sel.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (len(sel), 3) and residual.dtype == np.uint8
    assert np.all(np.diff(sel) > 0) and len(sel) <= max_selected
    if coverage is None:
        def coverage(recs):
            return case.coverage(recs=recs, radius=radius, bin_tolerance=bin_tolerance, margin=margin)[:2]
    c, r = coverage(case.recs[sel])
    assert np.asarray(r).tobytes() == residual.tobytes() and np.array_equal(c, counts[:, :2])
    assert int(counts[:, 2].sum()) == int((residual != labels).sum())
    assert len(sel) == 0 or counts[0, 2] == counts[0, 1]
    assert np.all(counts[:, 2] >= min_pixels) and np.all(1000 * counts[:, 2].astype(np.int64) >= SR.permille(min_new) * counts[:, 1])
    assert np.all(1000 * counts[:, 1].astype(np.int64) >= SR.permille(min_coverage) * counts[:, 0])
    keyed = [case.recs["transform"][j].tobytes() + case.recs["tmpl_idx"][j].tobytes() for j in sel]
    assert len(set(keyed)) == len(keyed)                                         # a duplicate of an accepted record is never accepted
    if SR.permille(min_new) == 1000:
        assert np.array_equal(counts[:, 2], counts[:, 1]) and int(counts[:, 1].sum()) == int((residual != labels).sum())
