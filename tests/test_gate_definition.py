"""The gate inside the minimum by its numpy statement (gate_ref.py) on hand-made cost arrays: no device, no library.  What
the statement must say before anything is held to it: a point whose unrestricted best pair fails the gate goes to the best
pair that passes; min_matched = 0 changes nothing; a NaN cost is never matched; an infinite cost under a cap of +inf is; a
template whose lengths sum to 0 passes any gate."""
import numpy as np

from capped_ref import capped_volumes
from detect_all_ref import detect_all_ref
from detect_ref import best_ref
from gate_ref import gated_best, gated_q, gated_volumes, pair_matched_lengths, passes
from matched_ref import gated, need, totals

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)


def _world(cost, offsets, caps, lens):
    """Hand-made line costs (L, 1, ny, nx) as a scene: the capped scores (penalty None: q is the score) and ML."""
    cost = np.asarray(cost, dtype=np.float32)
    offsets = np.asarray(offsets, dtype=np.int64)
    T = len(offsets) - 1
    adm = np.zeros((T,) + cost.shape[1:], dtype=np.float32)  # every pose admissible
    q = capped_volumes(cost, offsets, caps, adm)
    ml = pair_matched_lengths(cost, offsets, caps, lens)
    return q, ml


def _two_views():
    """Two templates of four lines of length 1, caps 3, on a grid of 1 x 3.  Point 0: the wrong view (template 0) matches two
    lines perfectly and has two capped (q = 6, half matched); the right view (template 1) matches all four moderately (q =
    8).  Point 1: both pass, the first wins.  Point 2: neither passes at min_matched 0.75."""
    wrong = [[0, 1, 9], [0, 1, 9], [9, 1, 9], [9, 1, 1]]
    right = [[2, 2, 9], [2, 2, 9], [2, 2, 1], [2, 2, 9]]
    cost = np.array(wrong + right, dtype=np.float32).reshape(8, 1, 1, 3)
    caps = [np.full(4, 3, dtype=np.float32)] * 2
    lens = [np.ones(4, dtype=np.float32)] * 2
    return cost, [0, 4, 8], caps, lens


def test_a_point_whose_best_pair_fails_goes_to_the_second_pair():
    cost, off, caps, lens = _two_views()
    q, ml = _world(cost, off, caps, lens)
    assert q[:, 0, 0].tolist() == [[6, 4, 10], [8, 8, 10]]
    assert ml[:, 0, 0].tolist() == [[2, 4, 1], [4, 4, 1]]
    s0, p0 = best_ref(q)
    assert p0.tolist() == [[0, 0, 0]]
    # gate WINNER: the winner of point 0 fails and the point is lost
    tl = totals(lens)
    sw, pw = gated(s0, p0, ml.reshape(2, 1, 3)[p0, 0, np.arange(3)].reshape(1, 3), need(0.75, np.repeat(tl, 1)))
    assert pw.tolist() == [[-1, 0, -1]]
    # gate ALL: point 0 goes to the right view with the right view's score and fraction
    s, p, fr = gated_best(q, ml, 0.75, lens)
    assert p.tolist() == [[1, 0, -1]]
    assert s[0, :2].tolist() == [8, 4] and np.isnan(s[0, 2])
    assert fr[0, :2].tolist() == [1, 1] and np.isnan(fr[0, 2])
    # and the records follow the planes: two detections at overlap 1, in score order
    boxes = np.array([[0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    rec, F = detect_all_ref(s, p, boxes, (0, 0, 3, 1, 1, 1), np.inf, 8, 1000)
    assert rec["score"].tolist() == [4, 8] and rec["tmpl_idx"].tolist() == [0, 1]
    assert rec["transform"][:, 2].tolist() == [1, 0]


def test_min_matched_zero_changes_nothing():
    cost, off, caps, lens = _two_views()
    q, ml = _world(cost, off, caps, lens)
    assert gated_q(q, ml, 0.0, totals(lens)).tobytes() == q.tobytes()
    s, p, fr = gated_best(q, ml, 0.0, lens)
    s0, p0 = best_ref(q)
    assert s.tobytes() == s0.tobytes() and p.tobytes() == p0.tobytes()
    assert fr.tolist() == [[0.5, 1, 0.25]]


def test_nan_infinity_and_zero_length():
    # one template of two lines of lengths 1 and 3; need at min_matched 1 is TL = 4
    lens = [np.array([1, 3], dtype=np.float32)]
    off = [0, 2]
    cost = np.array([[1, 1, INF, 1], [1, NAN, 1, 9]], dtype=np.float32).reshape(2, 1, 1, 4)
    # a NaN cost is never matched, not even under a cap of +inf; an infinite cost under a cap of +inf is
    caps = [np.array([INF, INF], dtype=np.float32)]
    q, ml = _world(cost, off, caps, lens)
    assert ml[0, 0, 0].tolist() == [4, 1, 4, 4]
    ok = passes(ml, 1.0, totals(lens))[0, 0, 0]
    assert ok.tolist() == [True, False, True, True]
    s, p, fr = gated_best(q, ml, 1.0, lens)
    assert p.tolist() == [[0, -1, 0, 0]] and s[0, 2] == INF and s[0, 3] == 10
    # a NaN q is no candidate whatever its ML: min_matched 0 does not bring point 1 back
    assert gated_best(q, ml, 0.0, lens)[1].tolist() == [[0, -1, 0, 0]]
    # finite caps: the infinite cost is capped in the score and not matched
    caps = [np.array([5, 5], dtype=np.float32)]
    q, ml = _world(cost, off, caps, lens)
    assert ml[0, 0, 0].tolist() == [4, 1, 3, 1] and q[0, 0, 0, 2] == 6
    assert gated_best(q, ml, 0.75, lens)[1].tolist() == [[0, -1, 0, -1]]
    # a cap of 0 is met by a cost of 0 only
    caps = [np.array([0, 5], dtype=np.float32)]
    zero = np.array([[0, 1], [1, 1]], dtype=np.float32).reshape(2, 1, 1, 2)
    assert _world(zero, off, caps, lens)[1][0, 0, 0].tolist() == [4, 3]
    # TL = 0: need = 0 and ML = 0 pass every gate; the fraction is 1
    flat = [np.zeros(2, dtype=np.float32)]
    q, ml = _world(cost, off, [np.array([0.5, 0.5], dtype=np.float32)], flat)
    s, p, fr = gated_best(q, ml, 1.0, flat)
    assert p.tolist() == [[0, -1, 0, 0]] and fr[0, [0, 2, 3]].tolist() == [1, 1, 1]


def test_windows_volumes_lose_the_failing_poses_only():
    cost, off, caps, lens = _two_views()
    q, ml = _world(cost, off, caps, lens)
    vols = [q[0], None]
    out = gated_volumes(vols, ml, 0.75, lens)
    assert out[1] is None and np.isnan(out[0][0, 0, [0, 2]]).all() and out[0][0, 0, 1] == 4
    assert gated_volumes(vols, ml, 0.0, lens)[0].tobytes() == q[0].tobytes()
