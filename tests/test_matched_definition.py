"""The numpy referee of the matched fraction (matched_ref.py) against the rule of include/fdcm.h, "Detections by matched
fraction", stated point by point in Python: caps of 0 and +inf, costs of 0, inf and NaN, lines of length zero, a template
without lines, and the properties the definition promises.  No device, no library."""
import numpy as np

from matched_ref import fractions, gated, matched_lengths, need, total, totals

f32 = np.float32
INF = f32(np.inf)
NAN = f32(np.nan)


def _brute_ml(cost, caps, lens):
    """ML of one point: line by line, in order, from +0."""
    ml = f32(0)
    for c, cap, ln in zip(cost, caps, lens):
        if not np.isnan(c) and f32(c) <= f32(cap):
            ml = f32(ml + f32(ln))
    return ml


def _inputs(rng, n, pts):
    """Costs (n, pts), caps (n,) and lengths (n,) with every special value of the definition among them."""
    cost = (rng.uniform(0, 1, (n, pts)) * 10.0 ** rng.uniform(-2, 3, (n, pts))).astype(np.float32)
    r = rng.uniform(size=cost.shape)
    cost[r < 0.10] = 0
    cost[(r >= 0.10) & (r < 0.17)] = INF
    cost[(r >= 0.17) & (r < 0.24)] = NAN
    caps = (rng.uniform(0, 1, n) * 10.0 ** rng.uniform(-2, 3, n)).astype(np.float32)
    r = rng.uniform(size=n)
    caps[r < 0.2] = 0
    caps[(r >= 0.2) & (r < 0.4)] = INF
    lens = rng.uniform(0, 50, n).astype(np.float32)
    lens[rng.uniform(size=n) < 0.15] = 0
    return cost, caps, lens


def test_matched_lengths_point_by_point():
    rng = np.random.default_rng(41)
    seen = {"zero cap met": 0, "zero cap missed": 0, "inf under inf": 0, "nan": 0, "inf over cap": 0}
    for n in [0, 1, 2, 3, 7, 8, 33, 70]:
        for _ in range(6):
            cost, caps, lens = _inputs(rng, n, 57)
            ml = matched_lengths(cost, caps, lens)
            assert ml.dtype == np.float32 and ml.shape == (57,)
            tl = total(lens)
            for p in range(57):
                want = _brute_ml(cost[:, p], caps, lens)
                assert ml[p].tobytes() == want.tobytes()
                assert 0 <= ml[p] <= tl
            for i in range(n):
                seen["zero cap met"] += int(((caps[i] == 0) & (cost[i] == 0)).sum())
                seen["zero cap missed"] += int(((caps[i] == 0) & (cost[i] > 0)).sum())
                seen["inf under inf"] += int(((caps[i] == INF) & (cost[i] == INF)).sum())
                seen["inf over cap"] += int(((caps[i] < INF) & (cost[i] == INF)).sum())
                seen["nan"] += int(np.isnan(cost[i]).sum())
    assert all(v > 20 for v in seen.values()), seen


def test_the_compare_is_the_rule():
    """One line of length 3: a cost equal to the cap is matched, the next float above is not; NaN is never matched, not even
    under +inf; inf is matched under +inf alone; a cap of 0 is met by +0 and -0 only."""
    L = f32([3])
    ml = lambda c, cap: matched_lengths(f32([[c]]), f32([cap]), L)[0]
    assert ml(2.5, 2.5) == 3 and ml(np.nextafter(f32(2.5), INF), 2.5) == 0
    assert ml(NAN, INF) == 0 and ml(NAN, 0) == 0
    assert ml(INF, INF) == 3 and ml(INF, np.finfo(np.float32).max) == 0
    assert ml(0.0, 0) == 3 and ml(-0.0, 0) == 3 and ml(np.array([1], dtype=np.uint32).view(np.float32)[0], 0) == 0
    # the sum is sequential in float32: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 does not
    big = f32(2.0 ** 24)
    assert matched_lengths(np.zeros((3, 1), dtype=np.float32), f32([1, 1, 1]), f32([big, 1, 1]))[0] == big
    assert matched_lengths(np.zeros((3, 1), dtype=np.float32), f32([1, 1, 1]), f32([1, 1, big]))[0] == big + f32(2)


def test_totals_and_fractions():
    rng = np.random.default_rng(43)
    for n in [0, 1, 5, 70]:
        cost, caps, lens = _inputs(rng, n, 40)
        tl = total(lens)
        assert tl.dtype == np.float32 and tl == matched_lengths(np.zeros((n, 1), dtype=np.float32), np.full(n, INF, dtype=np.float32), lens)[0]
        every = np.zeros((n, 40), dtype=np.float32)  # cost 0 meets every cap
        assert np.all(matched_lengths(every, caps, lens) == tl)
        assert np.all(fractions(matched_lengths(every, caps, lens), tl) == 1)
        fr = fractions(matched_lengths(cost, caps, lens), tl)
        assert fr.dtype == np.float32 and np.all((fr >= 0) & (fr <= 1))
        if tl > 0:
            ml = matched_lengths(cost, caps, lens)
            assert fr.tobytes() == (ml / tl).astype(np.float32).tobytes()
    # a template without lines, and one with lines of length zero only: TL = 0 and frac = 1 whatever is matched
    assert total(np.zeros(0)) == 0 and fractions(f32(0), f32(0)) == 1
    zl = np.zeros(4, dtype=np.float32)
    for c in (0.0, 5.0, np.nan):
        assert fractions(matched_lengths(np.full((4, 3), c, dtype=np.float32), f32([1, 1, 1, 1]), zl), total(zl)).tolist() == [1, 1, 1]
    assert totals([np.zeros(0), f32([1, 2]), zl]).tolist() == [0, 3, 0]


def test_the_gate():
    """need = float32(min_matched * TL); min_matched = 1 passes exactly when ML == TL, 0 passes everything with a candidate;
    points without a candidate stay as they are; gated points become NaN / -1."""
    rng = np.random.default_rng(47)
    sets = [_inputs(rng, n, 63) for n in (1, 4, 9, 0, 3)]
    sets[4] = (sets[4][0], sets[4][1], np.zeros(3, dtype=np.float32))  # lengths of zero only
    tl = totals([s[2] for s in sets])
    pairs = rng.integers(-1, len(sets), 63).astype(np.int32).reshape(7, 9)
    scores = np.where(pairs >= 0, rng.uniform(0, 3, (7, 9)), np.nan).astype(np.float32)
    ml = np.zeros(63, dtype=np.float32)
    for u, (cost, caps, lens) in enumerate(sets):
        here = pairs.reshape(-1) == u
        ml[here] = matched_lengths(cost, caps, lens)[here]
    ml = ml.reshape(7, 9)
    assert need(1.0, tl).tobytes() == tl.tobytes() and np.all(need(0.0, tl) == 0)
    assert need(0.3, tl).tobytes() == (f32(0.3) * tl).astype(np.float32).tobytes()
    s0, p0 = gated(scores, pairs, ml, need(0.0, tl))
    assert s0.tobytes() == scores.tobytes() and np.array_equal(p0, pairs)
    s1, p1 = gated(scores, pairs, ml, need(1.0, tl))
    full = ml == tl[np.where(pairs >= 0, pairs, 0)]
    assert np.array_equal(p1 >= 0, (pairs >= 0) & full) and np.array_equal(np.isnan(s1), p1 < 0)
    assert np.array_equal(p1[p1 >= 0], pairs[p1 >= 0]) and ((p1 < 0) & (pairs >= 0)).any() and (p1 >= 0).any()
    for mm in (0.25, 0.5, 0.9):
        s, p = gated(scores, pairs, ml, need(mm, tl))
        for j in range(7):
            for i in range(9):
                u = pairs[j, i]
                keep = u >= 0 and ml[j, i] >= f32(f32(mm) * tl[u])
                assert (p[j, i] == u and s[j, i] == scores[j, i]) if keep else (p[j, i] == -1 and np.isnan(s[j, i]))
    # a pair whose template has no length passes every gate: need = 0
    assert np.all(gated(scores, pairs, ml, need(1.0, tl))[1][(pairs == 3) | (pairs == 4)] >= 3)
