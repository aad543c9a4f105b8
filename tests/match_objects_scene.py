"""The end-to-end scenes of the match lists with objects and hull shapes.  Not collected: the tests import it.

two_rods        two parallel 60 x 10 rods at 45 degrees, 16 pixels apart along their normal, and one rod template.  Their boxes
                have IoU 0.42 and the rods share no pixel: search -> detect_matches(overlap 0.3) leaves one rod, and
                detect_matches_objects on the hull list leaves two.
washer_in_plate a 40 x 40 plate and a 26 x 26 washer lying inside it, two templates and two objects.  The washer's box is 0.42
                of the plate's: it is kept at cross_overlap 0.8 and dropped at cross_overlap = overlap = 0.3.

test_match_objects_scene.py confirms both on the CPU, with the oracle's match list and the referee, before
test_gpu_match_objects.py asks them of the device.  MAX_SCORE lies between the q of the true poses and the best junk's."""
import numpy as np

MAX_TMPL, MAX_SCENE = 4, 10
DEPTH, COEFF, PADDING = 30, 5.0, 2.2
ROD = np.float64([[0, 0], [60, 0], [60, 10], [0, 10]])
ROD_ANGLE, ROD_AT, ROD_GAP = np.pi / 4, (60.0, 20.0), 16.0
ROD_MAX_SCORE = 0.4   # the oracle's list: the records on the two rods have q 0.255 and 0.283, the best junk (6 pixels off) 0.477
PLATE = np.float64([[0, 0], [40, 0], [40, 40], [0, 40]])
WASHER = np.float64([[0, 0], [26, 0], [26, 26], [0, 26]])
PLATE_AT, WASHER_AT = (0.3, 50.0, 30.0), (0.3, 55.0, 38.5)
PLATE_MAX_SCORE = 1.0   # the oracle's list: the plate has q 0.294, the washer 0.407, the best junk 8.1
CLUTTER = np.float64([[5, 140, 40, 150], [150, 10, 158, 60], [130, 150, 158, 152], [2, 2, 20, 4]])


def polygon_lines(pts):
    pts = np.asarray(pts, dtype=np.float64)
    return np.concatenate([pts, np.roll(pts, -1, axis=0)], axis=1).T      # (4, N): x1, y1, x2, y2


def posed(part, angle, x, y):
    c, s = np.cos(angle), np.sin(angle)
    return np.asarray(part) @ np.array([[c, s], [-s, c]]) + np.array([x, y])


def two_rods():
    """(scene (4, N) float32, templates, the two rods' centres in the scene)"""
    nx, ny = -np.sin(ROD_ANGLE), np.cos(ROD_ANGLE)
    inst = [posed(ROD, ROD_ANGLE, ROD_AT[0] + k * ROD_GAP * nx, ROD_AT[1] + k * ROD_GAP * ny) for k in (0, 1)]
    scene = np.concatenate([polygon_lines(q) for q in inst] + [CLUTTER.T], axis=1).astype(np.float32)
    return scene, [polygon_lines(ROD).astype(np.float32)], [tuple(q.mean(axis=0)) for q in inst]


def washer_in_plate():
    """(scene, templates [plate, washer], objects, the two centres)"""
    inst = [posed(PLATE, *PLATE_AT), posed(WASHER, *WASHER_AT)]
    scene = np.concatenate([polygon_lines(q) for q in inst] + [CLUTTER.T], axis=1).astype(np.float32)
    return scene, [polygon_lines(PLATE).astype(np.float32), polygon_lines(WASHER).astype(np.float32)], [0, 1], [tuple(q.mean(axis=0)) for q in inst]


def centre_of(tmpl, transform):
    """The centre of a template's end points under a record's transform."""
    t = np.asarray(tmpl, dtype=np.float64).reshape(4, -1)
    M = np.asarray(transform, dtype=np.float64).reshape(2, 3)
    pts = np.concatenate([t[:2], t[2:]], axis=1)
    return tuple((M[:, :2] @ pts + M[:, 2:3]).mean(axis=1))
