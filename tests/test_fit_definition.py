"""The referee of the pose fit (tests/fit_ref.py; include/fdcm.h, "Match lists: pose fit") against the section's statements, on
the referee alone: the fit pixels are a subset of what match_coverage_ref explains and equal a count made by plain loops; an
integer rectangle on its own exact labels does not move; the labels shifted by whole pixels move it by exactly that; every
status is reached by a constructed record; permuting the list permutes the rows.  No device."""
import numpy as np

import coverage_ref as CR
import fit_cases as FC
import fit_ref as FR
import match_coverage_ref as MC
import match_ref as MR
from edge_ref import keys_of

f32 = np.float32
KEYS = keys_of(6)                      # slice 0 is vertical, slice 3 horizontal
RECT = [[10, 10], [50, 10], [50, 40], [10, 40]]


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).shape == np.asarray(y).shape
               and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def rect_labels(width, height, rect, dx=0, dy=0, edges=(0, 1, 2, 3)):
    """The pixels of the integer rectangle's edges (corners included), moved by (dx, dy) and cut to the image, each with its
    line's bin: horizontal edges 3, vertical ones 0."""
    lab = np.full((height, width), 255, dtype=np.uint8)
    pts = np.asarray(rect, dtype=np.int64)
    for i in edges:
        (x1, y1), (x2, y2) = pts[i], pts[(i + 1) % 4]
        k = max(abs(x2 - x1), abs(y2 - y1)) + 1
        xs, ys = np.linspace(x1, x2, k).astype(np.int64) + dx, np.linspace(y1, y2, k).astype(np.int64) + dy
        ok = (xs >= 0) & (xs < width) & (ys >= 0) & (ys < height)
        lab[ys[ok], xs[ok]] = 3 if y1 == y2 else 0
    return lab


def rect_fit(lab, M=(1, 0, 0, 0, 1, 0), rect=RECT, **kw):
    tm = [FC.polygon_lines(rect).astype(np.float32)]
    rec = MR.records([0], [7.5], [M])
    par = dict(radius=3, bin_tolerance=0, iterations=1, damping=0.0)
    par.update(kw)
    return rec, FR.fit(lab, KEYS, (0, 0), lab.shape[1], lab.shape[0], tm, rec, **par)


def test_a_fit_pixels_are_explained_pixels_and_a_plain_count():
    w = FC.world("b5-d6")
    recs = np.concatenate([w.recs[:2], w.recs[20:22], w.recs[30:32], w.recs[100:108], w.recs[150:156], w.recs[-14:]])
    lines = np.array([w.tmpls[t].shape[1] if 0 <= t < len(w.tmpls) else 0 for t in recs["tmpl_idx"].astype(np.int64) - w.base])
    for radius, tol in [(0, 0), (3, 1), (32, w.m // 2)]:
        _, info, _ = w.ref(radius, tol, 1, recs=recs)
        counts = MC.coverage(w.labels, w.keys, w.T, w.W, w.H, w.tmpls, recs, w.base, radius=radius, bin_tolerance=tol)[0]
        adm = counts[:, 0] >= 0
        assert np.array_equal(info[:, 0] == -1, ~adm) and adm.sum() >= 20 and (~adm).sum() >= 5
        assert np.all(info[adm, 2] <= counts[adm, 1]) and np.all(info[~adm, 2] == 0)
        assert radius == 0 or np.any(info[adm, 2] < counts[adm, 1])            # the end caps explain, and take no part
        # the count by loops over pixels and lines, written out here (the templates of up to 64 lines)
        for j in np.flatnonzero(adm & (lines <= 64)):
            _, ends, bins, _ = MC.segments(w.keys, w.T, w.W, w.H, w.tmpls, recs[j], w.base)
            x0, y0, x1, y1 = MC.window(w.tmpls, recs[j], w.base, radius, w.width, w.height)
            n = 0
            for y in range(y0, y1 + 1):
                for x in range(x0, x1 + 1):
                    if w.labels[y, x] >= w.m:
                        continue
                    for i in range(ends.shape[1]):
                        ax, ay, bx, by = (int(v) - w.border for v in ends[:, i])
                        dx, dy, wx, wy = bx - ax, by - ay, x - ax, y - ay
                        dot, len2, cross = wx * dx + wy * dy, dx * dx + dy * dy, wx * dy - wy * dx
                        if int(CR.bin_distance(int(w.labels[y, x]), int(bins[i]), w.m)) <= tol and 0 < dot < len2 and cross * cross <= radius * radius * len2:
                            n += 1
                            break
            assert n == info[j, 2], (radius, tol, j, n, info[j])
    # the moments by plain loops and by arrays are the same integers: the whole result agrees
    some = recs[lines <= 65]
    assert same(w.ref(3, 1, 2, recs=some, plain=True), w.ref(3, 1, 2, recs=some))


def test_b_an_integer_rectangle_on_its_own_labels_stays():
    lab = rect_labels(64, 56, RECT)
    for it in (1, 3):
        rec, (out, info, rms) = rect_fit(lab, iterations=it, damping=1e-3)
        assert out.tobytes() == rec.tobytes()
        n = 2 * 39 + 2 * 29                                     # the pixels strictly inside each edge
        assert info.tolist() == [[0, it, n, n]] and rms.tolist() == [[0.0, 0.0]]


def test_c_whole_pixel_shifts_are_recovered_exactly():
    lab = rect_labels(64, 56, RECT, 2, -1)
    rec, (out, info, rms) = rect_fit(lab)
    M = out["transform"][0]
    assert info[0, 0] == 0 and info[0, 1] == 1 and info[0, 2] > 100
    assert M[2] == f32(2) and M[5] == f32(-1) and abs(float(M[1])) < 1e-12 and abs(float(M[3])) < 1e-12
    assert M[0] == f32(1) and M[4] == f32(1) and out["score"][0] == f32(7.5) and out["tmpl_idx"][0] == 0
    assert rms[0, 0] > 1.0 and rms[0, 1] < 1e-6
    # from a non-integer start the same labels bring it to the same place
    rec, (out, info, rms) = rect_fit(lab, M=(1, 0, 0.4, 0, 1, 0.3), iterations=2)
    assert info[0, 0] == 0 and np.abs(out["transform"][0] - f32([1, 0, 2, 0, 1, -1])).max() < 1e-5


def test_d_every_status_is_reached():
    lab = rect_labels(64, 56, RECT, 2, -1)
    # 0 and -1: the fit above, and the record moved off the map
    rec, (out, info, rms) = rect_fit(lab, M=(1, 0, -11, 0, 1, 0))
    assert info.tolist() == [[-1, 0, 0, 0]] and np.all(np.isnan(rms)) and out.tobytes() == rec.tobytes()
    rec = MR.records([1], [0], [[1, 0, 0, 0, 1, 0]])
    out, info, rms = FR.fit(lab, KEYS, (0, 0), 64, 56, [FC.polygon_lines(RECT).astype(np.float32)], rec)
    assert info.tolist() == [[-1, 0, 0, 0]] and np.all(np.isnan(rms)) and out.tobytes() == rec.tobytes()
    # 1: too few pixels -- none on blank labels (rms NaN), some with a large min_pixels
    rec, (out, info, rms) = rect_fit(np.full((56, 64), 255, dtype=np.uint8))
    assert info.tolist() == [[1, 0, 0, 0]] and np.all(np.isnan(rms)) and out.tobytes() == rec.tobytes()
    rec, (out, info, rms) = rect_fit(lab, min_pixels=1000)
    assert info[0, 0] == 1 and info[0, 1] == 0 and 100 < info[0, 2] == info[0, 3] < 1000 and rms[0, 0] == rms[0, 1] > 1 and out.tobytes() == rec.tobytes()
    # 2: one horizontal line fixes no x: without damping the first pivot is zero
    line = [np.float32([[10], [20], [50], [20]])]
    hl = np.full((56, 64), 255, dtype=np.uint8)
    hl[21, 5:60] = 3
    rec = MR.records([0], [0], [[1, 0, 0, 0, 1, 0]])
    out, info, rms = FR.fit(hl, KEYS, (0, 0), 64, 56, line, rec, radius=3, bin_tolerance=0, iterations=2, damping=0.0)
    assert info.tolist() == [[2, 0, 39, 39]] and rms.tolist() == [[1.0, 1.0]] and out.tobytes() == rec.tobytes()
    # 3: a step longer than max_shift, or a turn larger than max_angle
    rec, (out, info, rms) = rect_fit(lab, max_shift=1.5)
    assert info[0, 0] == 3 and info[0, 1] == 0 and out.tobytes() == rec.tobytes()
    rec, (out, info, rms) = rect_fit(lab, max_shift=2.5)
    assert info[0, 0] == 0 and info[0, 1] == 1
    rec, (out, info, rms) = rect_fit(lab, max_angle=0.0)
    assert info[0, 0] in (0, 3)                                            # (the turn is rounding noise, or exactly zero)
    # 4: the step would carry the right edge to x = 64 = W: it is not taken, and the first pass's figures stand
    rect = [[10, 10], [51, 10], [51, 40], [10, 40]]
    lab4 = rect_labels(64, 56, rect, 10 + 3, 0)
    rec, (out, info, rms) = rect_fit(lab4, M=(1, 0, 10, 0, 1, 0), rect=rect, radius=4, iterations=2)
    assert info[0, 0] == 4 and info[0, 1] == 0 and info[0, 2] == info[0, 3] > 50 and rms[0, 0] == rms[0, 1] > 0 and out.tobytes() == rec.tobytes()
    rec, (out, info, rms) = rect_fit(rect_labels(64, 56, rect, 10 + 2, 0), M=(1, 0, 10, 0, 1, 0), rect=rect, radius=4, iterations=2)
    assert info[0, 0] == 0 and info[0, 1] == 2 and out["transform"][0, 2] == f32(12)      # one pixel less: inside, and taken


def test_e_permuting_the_list_permutes_the_rows():
    w = FC.world("b0-d30")
    recs = np.concatenate([w.recs[:8], w.recs[40:60], w.recs[-10:]])
    out, info, rms = w.ref(3, 1, 2, recs=recs)
    perm = np.random.default_rng(2).permutation(len(recs))
    got = w.ref(3, 1, 2, recs=recs[perm])
    assert same(got, (out[perm], info[perm], rms[perm])) and len(set(info[:, 0].tolist())) >= 3
