"""CPU-only checks of the hull footprints (include/fdcm.h, "Hull footprints") that need no device: the two statements of the
shape in hull_ref.py agree with each other and with fdcm_lines_footprint_spans int for int, the consequences the header
states hold, and the rod table of the README is reproduced from the referees."""
import ctypes as C
import os

import numpy as np
import pytest

import hull_ref as hr
from nms_ref import box_of_lines, footprints

f32 = np.float32
MARGINS = (0, 1, 7)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def lines(*segs):
    return np.array(segs, dtype=np.float32).reshape(-1, 4).T.copy()


def degenerate():
    return {
        "one line": lines((1.5, 2.5, 9.2, 6.9)),
        "zero length": lines((3.7, -2.2, 3.7, -2.2)),
        "collinear": lines((0, 0, 4, 2), (8, 4, 12, 6), (-4, -2, 2, 1)),
        "thin diagonal": lines((0.0, 0.0, 3.0, 11.0)),
        "horizontal": lines((-3.5, 2.0, 7.5, 2.0)),
        "vertical": lines((2.0, -5.0, 2.0, 5.0)),
        "nan": lines((0, 0, 4, 2), (1, np.nan, 2, 2)),
        "no lines": np.zeros((4, 0), dtype=np.float32),
        "triangle": lines((0, 0, 6, 0), (6, 0, 0, 4), (0, 4, 0, 0)),
        "negative": lines((-9.5, -3.2, -1.1, -7.9), (-4.4, -0.5, -6.0, -8.8)),
    }


def random_templates(seed, count=12):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(1, 7))
        out.append((rng.uniform(-14, 14, size=(4, n)) * (1 + i % 3)).astype(np.float32))
    return out


def table():
    a = np.deg2rad([0, 45, 90, 135, 180, 225, 270, 315])
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def c_spans(capi, tmpls, cs=None, pivots=None, margin=0):
    from openfdcm_amd.engine import lines_footprint_spans
    return lines_footprint_spans(tmpls, cs, pivots, margin=margin)


@pytest.mark.parametrize("margin", MARGINS)
def test_the_statements_agree_on_degenerate_templates(margin):
    for name, tm in degenerate().items():
        v = hr.vertices(tm, margin)
        a, b, c = hr.rows_by_pairs_exact(v), hr.rows_by_pairs(v), hr.rows_by_halfplanes(v)
        assert hr._same_rows(a, b) and hr._same_rows(a, c), name
        assert (len(v) == 0) == (name in ("nan", "no lines"))
        if v:
            assert sum(max(0, r - l + 1) for l, r in a.values()) >= 1  # A(u) >= 1
    thin = hr.rows_by_pairs_exact(hr.vertices(degenerate()["thin diagonal"], 0))
    assert sum(l > r for l, r in thin.values()) >= 5  # the segment passes between lattice points
    assert all(l > r for y, (l, r) in thin.items() if y not in (0, 11))


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("rot", [False, True])
def test_the_statements_agree_on_random_templates(margin, rot):
    tmpls = random_templates(5 + margin)[:6]
    cs = table() if rot else None
    piv = np.array([[1.5, -2.0]] * len(tmpls), dtype=np.float32) if rot else None
    n = 0
    for row in hr.posed(tmpls, cs, piv):
        for l in row[::3]:
            v = hr.vertices(l, margin)
            a = hr.rows_by_pairs(v)
            assert hr._same_rows(a, hr.rows_by_halfplanes(v))
            if margin == 0:
                assert hr._same_rows(a, hr.rows_by_pairs_exact(v))
            n += 1
    assert n >= 6


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("rot", [False, True])
def test_the_library_gives_the_referees_table(capi, margin, rot):
    tmpls = list(degenerate().values()) + random_templates(11)
    cs = table() if rot else None
    piv = None
    if rot:
        piv = np.zeros((len(tmpls), 2), dtype=np.float32)
        piv[::2] = [3.25, -1.5]
    off, spans, areas = c_spans(capi, tmpls, cs, piv, margin)
    want = hr.span_table(hr.shapes(tmpls, cs, piv, margin))
    assert off.dtype == np.int64 and spans.dtype == np.int32 and areas.dtype == np.int64
    assert np.array_equal(off, want[0]) and np.array_equal(spans, want[1]) and np.array_equal(areas, want[2])
    # the box of the spans is the box of fdcm_lines_footprints, which is the referee's
    from openfdcm_amd.engine import lines_footprints
    boxes = lines_footprints(tmpls, cs, piv, margin=margin).reshape(-1, 4)
    assert np.array_equal(boxes, footprints(tmpls, cs, piv, margin).reshape(-1, 4))
    for u in range(len(boxes)):
        rows = spans[off[u]:off[u + 1]]
        x0, y0, x1, y1 = (int(v) for v in boxes[u])
        assert len(rows) == max(0, y1 - y0 + 1)
        if len(rows):
            full = rows[rows[:, 0] <= rows[:, 1]]
            assert full[:, 0].min() == 0 and full[:, 1].max() == x1 - x0 and areas[u] >= 1
            assert rows[0, 0] <= rows[0, 1] and rows[-1, 0] <= rows[-1, 1]  # the first and the last row hold a vertex
        else:
            assert areas[u] == 0
    # offsets and areas alone, and the handle's call, give the same
    from openfdcm_amd.engine import _rotations
    T = len(tmpls)
    flat, offs = capi.pack_templates(tmpls)
    r = _rotations(cs, piv, T)[0] if rot else None
    o2, a2 = np.zeros(len(off), dtype=np.int64), np.zeros(len(areas), dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    assert capi.lib().fdcm_lines_footprint_spans(capi.fptr(flat), i64(offs), T, C.byref(r) if r is not None else None, margin, i64(o2), i64(a2),
                                                 None) == 0
    assert np.array_equal(o2, off) and np.array_equal(a2, areas)
    o3 = np.zeros(len(off), dtype=np.int64)
    assert capi.lib().fdcm_lines_footprint_spans(capi.fptr(flat), i64(offs), T, C.byref(r) if r is not None else None, margin, i64(o3), None,
                                                 None) == 0
    assert np.array_equal(o3, off)


@pytest.mark.parametrize("margin", MARGINS)
def test_identity_3_shapes_that_hold_their_boxes_corners_are_full_rectangles(capi, margin):
    rng = np.random.default_rng(3)
    tmpls = []
    for _ in range(5):
        x0, y0 = rng.uniform(-9, 9, size=2)
        w, h = rng.uniform(3, 12, size=2)
        tmpls.append(lines((x0, y0, x0 + w, y0 + h), (x0 + w, y0, x0, y0 + h), (x0 + 1, y0 + 1, x0 + 2, y0 + 2)))
    quarter = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)
    for cs in (None, quarter):
        off, spans, areas = c_spans(capi, tmpls, cs, None, margin)
        boxes = footprints(tmpls, cs, None, margin).reshape(-1, 4)
        for u, b in enumerate(boxes):
            rows = spans[off[u]:off[u + 1]]
            assert (rows[:, 0] == 0).all() and (rows[:, 1] == b[2] - b[0]).all()
            assert areas[u] == (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
        assert [s.area for s in hr.shapes(tmpls, cs, None, margin)] == list(areas)


def rod(length, width, angle_deg, offset):
    """The outline of a rod as four lines, its axis through `offset` along its normal from the origin."""
    a = np.deg2rad(angle_deg)
    ax, nrm = np.array([np.cos(a), np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
    c = 200 + nrm * offset
    p = [c + sx * ax * length / 2 + sy * nrm * width / 2 for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    return lines(*[(p[i][0], p[i][1], p[(i + 1) % 4][0], p[(i + 1) % 4][1]) for i in range(4)])


ROD_TABLE = [(200, 20, 30, 0.599, 17), (120, 16, 24, 0.519, 22), (60, 10, 14, 0.471, 26)]


@pytest.mark.parametrize("length,width,gap,iou,fill", ROD_TABLE)
def test_the_rod_table(length, width, gap, iou, fill):
    """Two parallel rods at 45 degrees: their boxes overlap by more than the default limit, their shapes share no lattice
    point, and at 0 degrees the boxes do not meet either."""
    a, b = rod(length, width, 45, 0), rod(length, width, 45, gap)
    A, B = (int(v) for v in box_of_lines(a)), (int(v) for v in box_of_lines(b))
    A, B = list(A), list(B)
    inter = max(0, min(A[2], B[2]) - max(A[0], B[0]) + 1) * max(0, min(A[3], B[3]) - max(A[1], B[1]) + 1)
    union = (A[2] - A[0] + 1) * (A[3] - A[1] + 1) + (B[2] - B[0] + 1) * (B[3] - B[1] + 1) - inter
    Sa, Sb = hr.Shape(a), hr.Shape(b)
    print("box IoU", inter / union, "fill", Sa.area / ((A[2] - A[0] + 1) * (A[3] - A[1] + 1)))
    assert 1000 * inter > 300 * union
    assert abs(inter / union - iou) < 0.02
    assert abs(100 * Sa.area / ((A[2] - A[0] + 1) * (A[3] - A[1] + 1)) - fill) < 2
    assert hr.overlap(Sa, (0, 0), Sb, (0, 0)) == 0 and not (Sa.pixels() & Sb.pixels())
    a0, b0 = rod(length, width, 0, 0), rod(length, width, 0, gap)
    A0, B0 = box_of_lines(a0), box_of_lines(b0)
    assert min(A0[3], B0[3]) < max(A0[1], B0[1])  # box IoU 0 at 0 degrees


def test_known_answers_counted_by_hand():
    # the triangle (0, 0), (6, 0), (0, 4): rows y = 0 .. 4 hold x <= 6 - 1.5 y: 7, 5, 4, 2, 1 pixels
    tri = hr.Shape(lines((0, 0, 6, 0), (6, 0, 0, 4), (0, 4, 0, 0)))
    assert tri.box == (0, 0, 6, 4) and list(tri.xl) == [0] * 5 and list(tri.xr) == [6, 4, 3, 1, 0] and tri.area == 19
    # the square (3, 0), (6, 3), (3, 6), (0, 3), a rectangle rotated by 45 degrees: rows 1, 3, 5, 7, 5, 3, 1
    dia = hr.Shape(lines((3, 0, 6, 3), (3, 6, 0, 3)))
    assert dia.box == (0, 0, 6, 6) and list(dia.xl) == [3, 2, 1, 0, 1, 2, 3] and list(dia.xr) == [3, 4, 5, 6, 5, 4, 3] and dia.area == 25
    # with margin 1 every vertex becomes a 3 x 3 square's corners: the octagon has rows 3, 5, 7, 9, 9, 9, 7, 5, 3
    fat = hr.Shape(lines((3, 0, 6, 3), (3, 6, 0, 3)), margin=1)
    assert fat.box == (-1, -1, 7, 7) and [int(r - l + 1) for l, r in zip(fat.xl, fat.xr)] == [3, 5, 7, 9, 9, 9, 7, 5, 3] and fat.area == 57
    # a 2 x 5 rectangle rotated so that its long side runs along (2, 1): (0, 0), (4, 2), (3, 4), (-1, 2)
    rect = hr.Shape(lines((0, 0, 4, 2), (3, 4, -1, 2)))
    assert rect.box == (-1, 0, 4, 4) and rect.area == 14
    assert [(int(l), int(r)) for l, r in zip(rect.xl, rect.xr)] == [(1, 1), (1, 3), (0, 5), (2, 4), (4, 4)]
    # overlap of the triangle with itself shifted by (4, 0): rows share 3, 1, 0, .. pixels
    assert hr.overlap(tri, (0, 0), tri, (4, 0)) == 3 + 1 and hr.overlap(tri, (0, 0), tri, (7, 0)) == 0
    assert hr.overlap(tri, (0, 0), tri, (0, 0)) == tri.area
