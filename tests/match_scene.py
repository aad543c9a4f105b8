"""The end-to-end scene of the calls on match lists: two instances of one polygon part and a few clutter lines.  Not collected:
the tests import it.

test_match_scene.py confirms on the CPU, with the oracle's match list and the referee, what test_gpu_matches.py then asks of
the device: search -> detect_matches(overlap 0.3, DefaultPenalty, MAX_SCORE) leaves exactly two records, one per instance.
MAX_SCORE lies between the q of the true poses and the best junk's."""
import numpy as np

MAX_TMPL, MAX_SCENE = 4, 10
MAX_SCORE = 2.0   # the oracle's list: the records on the two instances have q 0.51 .. 1.41, the best junk (10 pixels off) 2.59
PART = np.float64([[0, 0], [34, 0], [34, 12], [20, 12], [20, 30], [8, 30], [8, 18], [0, 18]])   # an eight-sided part, about 34 x 30
POSES = ((0.35, 38.0, 30.0), (2.2, 118.0, 104.0))                                                # (angle, x, y) of the two instances
CLUTTER = np.float64([[5, 140, 40, 150], [150, 10, 158, 60], [70, 75, 95, 68], [10, 80, 22, 120], [130, 150, 158, 152], [2, 2, 20, 4]])


def polygon_lines(pts):
    pts = np.asarray(pts, dtype=np.float64)
    return np.concatenate([pts, np.roll(pts, -1, axis=0)], axis=1).T      # (4, N): x1, y1, x2, y2


def posed_polygon(angle, x, y):
    c, s = np.cos(angle), np.sin(angle)
    return PART @ np.array([[c, s], [-s, c]]) + np.array([x, y])


def two_parts():
    """(scene (4, N) float32, templates, the two instances' centres in the scene)"""
    inst = [posed_polygon(*p) for p in POSES]
    scene = np.concatenate([polygon_lines(q) for q in inst] + [CLUTTER.T], axis=1).astype(np.float32)
    return scene, [polygon_lines(PART).astype(np.float32)], [tuple(q.mean(axis=0)) for q in inst]


def centre_of(tmpl, transform):
    """The centre of a template's end points under a record's transform."""
    t = np.asarray(tmpl, dtype=np.float64).reshape(4, -1)
    M = np.asarray(transform, dtype=np.float64).reshape(2, 3)
    pts = np.concatenate([t[:2], t[2:]], axis=1)
    return tuple((M[:, :2] @ pts + M[:, 2:3]).mean(axis=1))
