"""The end-to-end scenes of scene selection on match lists: the L-shaped part with the bar lying in its notch.  Not collected:
the tests import it.

Templates are the part's and the bar's outlines, the scene lines are the two outlines in the frame, the labels are
edge_ref.edge_labels(frame, 30, 60) with the frame (0, 0).  The chain is search -> the detect rule at overlap 1 (the priority
order: ascending by key, what lies outside the map dropped) -> scene selection at min_new 0.25, 0.5 and 0.75.  "On a part" means
the centre of the posed template lies within 2 px of the part's centre.

Two places of the bar.  BAR_AT, select_cases.notch_frame's: two pixels from the part on both sides, for the chain on the CPU, on
the oracle's list of a map built from the scene lines.  What the referee returned there (test_match_coverage_scene.py asserts
it): 60 records, all of them candidates at overlap 1; at the three shares alike the records 0 and 4 of the priority order, the
bar with (edges, explained, new) = (42, 38, 38) and the part with (184, 137, 136); the box rule at overlap 0.25 keeps 7 records
of which one, on the bar, lies on a part: it loses the L-shaped part.
BAR_AT_IMAGE: three pixels from the part, for the chain on the device, whose map is built from the frame.  On that map the
search's best bar records sit 2.5 px towards the part, where image edges and outlines differ by the edge detector's offset.
With the bar two pixels away the device (and the referee on its records) returned at 0.25 the part and a bar record 2.5 px
off, (87, 80, 38), at 0.5 the part and the bar, (66, 59, 38), and at 0.75 the part and two junk records, because a bar pose
explains, at radius 2, 21 pixels of the part's edge two pixels away: not two clean parts.  Three pixels away it returned the
records 0 and 2, the part (222, 152, 152) and the bar (80, 76, 60), at the three shares alike.  (On the oracle's list the bar
three pixels away fails at 0.75, (80, 76, 38): each chain has the scene on which its list is clean; the rule and the
thresholds are the same.)"""
import numpy as np

import select_cases as SC
import test_gpu_coverage as G

MAX_TMPL, MAX_SCENE = 4, 4
SHARES = (0.25, 0.5, 0.75)
BOX_OVERLAP = 250   # the overlap the README cites for the box rule, in permille
BAR_AT = SC.BAR_AT
BAR_AT_IMAGE = (37, 61)   # three pixels from the part on both sides


def frame(bar_at=BAR_AT):
    """select_cases.notch_frame with the bar at bar_at: 160 x 120 at grey 60, the L-shaped part at 200 and the bar at 130 in its
    notch."""
    img = np.full((120, 160), 60, dtype=np.uint8)
    x0, y0 = G.PART_AT
    img[y0:y0 + 14, x0:x0 + 40] = 200
    img[y0 + 14:y0 + 34, x0:x0 + 16] = 200
    bx, by = bar_at
    img[by:by + 19, bx:bx + 23] = 130
    return img


def templates():
    return [G.part_template(), SC.outline(SC.BAR)]


def scene_lines(bar_at=BAR_AT):
    t = templates()
    return np.ascontiguousarray(np.concatenate([t[0] + np.float32([*G.PART_AT] * 2)[:, None], t[1] + np.float32([*bar_at] * 2)[:, None]], axis=1))


def centre_of(tmpl, transform):
    t = np.asarray(tmpl, dtype=np.float64).reshape(4, -1)
    M = np.asarray(transform, dtype=np.float64).reshape(2, 3)
    pts = np.concatenate([t[:2], t[2:]], axis=1)
    return (M[:, :2] @ pts + M[:, 2:3]).mean(axis=1)


def centres(bar_at=BAR_AT):
    """The centres of the part's and the bar's outlines in the frame."""
    t = templates()
    return [centre_of(t[0], [1, 0, G.PART_AT[0], 0, 1, G.PART_AT[1]]), centre_of(t[1], [1, 0, bar_at[0], 0, 1, bar_at[1]])]


def parts_of(recs, bar_at=BAR_AT):
    """Per record: 0 on the part, 1 on the bar (its own template, its centre within 2 px of the part's), -1 on neither."""
    t, c = templates(), centres(bar_at)
    out = []
    for r in recs:
        k = int(r["tmpl_idx"])
        d = centre_of(t[k], r["transform"]) - c[k]
        out.append(k if np.hypot(d[0], d[1]) <= 2.0 else -1)
    return out
