"""The meshes and views of the mesh-template tests, built in code (include/fdcm.h, "Templates from a mesh"): small solids and
sheets whose visible edges are known from geometry, and scales at which a rasteriser's lane / tile split and the two-pass
write can go wrong -- triangles that cover no pixel centre or exactly one, vertices on pixel centres (inclusive edges, ties
by face index), faces of 65 x 65, 256 x 3 and 257 x 3 pixels (and 3 x 256, 3 x 257) on either side of the small / large split, and
one of 2000; and meshes past one block per view: a bumped icosphere of 642 vertices (3 vertex blocks, the box set by vertices of
the later ones), 1280 faces and 1920 edges (8 edge blocks, lines in every one), and a fence whose two long edges are cut into 41
lines each by the slats in front of them."""
import numpy as np

COS30 = float(np.cos(np.deg2rad(30.0)))


def _quad(a, b, c, d):
    return [(a, b, c), (a, c, d)]


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)], dtype=np.float32)
    f = (_quad(0, 2, 3, 1) + _quad(4, 5, 7, 6) + _quad(0, 1, 5, 4) + _quad(2, 6, 7, 3) + _quad(0, 4, 6, 2) + _quad(1, 3, 7, 5))
    return v, np.array(f, dtype=np.int32)


def cube():
    return box_mesh((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32) * np.float32(0.5)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)


def triangle():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def open_square():
    v = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], dtype=np.float32)
    return v, np.array(_quad(0, 1, 2, 3), dtype=np.int32)


def prism(poly, z0, z1, tris):
    """A polygon (counter-clockwise, with its triangulation `tris`) extruded from z0 to z1."""
    n = len(poly)
    v = np.array([[x, y, z0] for x, y in poly] + [[x, y, z1] for x, y in poly], dtype=np.float32)
    f = [(a, c, b) for a, b, c in tris] + [(a + n, b + n, c + n) for a, b, c in tris]
    for i in range(n):
        j = (i + 1) % n
        f += _quad(i, j, j + n, i + n)
    return v, np.array(f, dtype=np.int32)


def l_prism():
    """An L: concave, both inner walls touch the edge above vertex 3."""
    poly = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    v, f = prism(poly, -0.5, 0.5, [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)])
    return v - np.array([1, 1, 0], dtype=np.float32), f


def notched_prism():
    """An L with a notch in its long arm: no symmetry, so no two views give the same template."""
    poly = [(0, 0), (3, 0), (3, 1), (2.2, 1), (2.2, 0.6), (1.7, 0.6), (1.7, 1), (1, 1), (1, 2), (0, 2)]
    tris = [(0, 1, 4), (1, 2, 3), (1, 3, 4), (0, 4, 5), (0, 5, 6), (0, 6, 7), (0, 7, 8), (0, 8, 9)]
    v, f = prism(poly, -0.4, 0.4, tris)
    return v - np.array([1.2, 0.8, 0], dtype=np.float32), f


def occluded_cubes():
    """A cube of side 2 and, in front of it (larger z), one of side 0.6 across the large one's edge x = 1."""
    v0, f0 = box_mesh((-1, -1, -1), (1, 1, 1))
    v1, f1 = box_mesh((0.7, -0.3, 1.5), (1.3, 0.3, 2.1))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + 8]).astype(np.int32)


def icosphere(subdivisions=2, bump=None):
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.sqrt(1 + t * t) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt(p @ p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    if bump is not None:
        v = v * bump(v)[:, None]
    return v.astype(np.float32), np.array(f, dtype=np.int32)


def bump3(p):
    return 1.0 + 0.25 * np.sin(5 * p[:, 0]) * np.cos(4 * p[:, 1])


def icosphere3_bumped():
    """642 vertices, 1280 faces, 1920 edges, 80 of them sharp at 30 degrees; concave in places."""
    return icosphere(3, bump3)


def fence(K=40):
    """An open sheet [0, 3K + 1] x [0, 1] at z = 0 (vertices 0 .. 3, counter-clockwise from (0, 0)) and K slats in front of it,
    [3k + 1.25, 3k + 2.75] x [-1, 2] at z = 1: the sheet's long edges (0, 1) and (2, 3) show in the K + 1 gaps."""
    v = [(0, 0, 0), (3 * K + 1, 0, 0), (3 * K + 1, 1, 0), (0, 1, 0)]
    f = _quad(0, 1, 2, 3)
    for k in range(K):
        n = len(v)
        v += [(3 * k + 1.25, -1, 1), (3 * k + 2.75, -1, 1), (3 * k + 2.75, 2, 1), (3 * k + 1.25, 2, 1)]
        f += _quad(n, n + 1, n + 2, n + 3)
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


def roof():
    """Two slopes that meet in the ridge (vertices 0, 1), each quad cut into two triangles: the triangle of a slope that does
    not hold the ridge lies in the plane of the one that does."""
    v = np.array([[-1, 0, 0.5], [1, 0, 0.5], [1, -1, 0], [-1, -1, 0], [1, 1, 0], [-1, 1, 0]], dtype=np.float32)
    return v, np.array(_quad(0, 3, 2, 1) + _quad(0, 1, 4, 5), dtype=np.int32)


def with_degenerate_faces():
    """A cube, a triangle of three collinear vertices and a face that names one vertex twice."""
    v, f = cube()
    v = np.concatenate([v, np.array([[2, 0, 0], [3, 0, 0], [4, 0, 0]], dtype=np.float32)])
    return v, np.concatenate([f, np.array([[8, 9, 10], [8, 8, 9]], dtype=np.int32)])


def non_manifold():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)


def rot(axis, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    m = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, dtype=np.float64)


def f32(m):
    return np.ascontiguousarray(m, dtype=np.float32)


IDENTITY = f32(np.eye(3))
GENERIC = f32(rot("x", -35.0) @ rot("y", 25.0))
GENERIC2 = f32(rot("z", 17.0) @ rot("x", 62.0) @ rot("y", -41.0))
SIDE = f32(rot("x", 90.0))                      # axis-aligned, the sheets edge-on
GRAZING = f32(rot("x", 90.0 - 26.565 - 2.0))    # two degrees off the roof's far slope (atan(0.5) = 26.565 degrees)
STRETCH_257 = f32(np.diag([256.5, 2.5, 1.0]))   # not orthonormal: the unit triangle becomes 257 x 3 pixels at scale 1
STRETCH_256 = f32(np.diag([255.5, 2.5, 1.0]))
TALL_257 = f32(np.diag([2.5, 256.5, 1.0]))      # 3 x 257 pixels: one column of tiles (tx == 1), 65 of them
TALL_256 = f32(np.diag([2.5, 255.5, 1.0]))      # 3 x 256: 64 tiles, the most the small path takes
FENCE_TURNED = f32(rot("z", 17.0))

MESHES = {"cube": cube, "tetrahedron": tetrahedron, "triangle": triangle, "open_square": open_square, "l_prism": l_prism,
          "occluded_cubes": occluded_cubes, "icosphere": icosphere, "roof": roof, "degenerate": with_degenerate_faces,
          "icosphere3_bumped": icosphere3_bumped, "fence": fence}

# (name, mesh, views, scale): what the GPU tests compare key for key and byte for byte
CASES = [
    ("cube-centres", "cube", [IDENTITY, GENERIC], 65.0),          # vertices on pixel centres, the diagonal through centres
    ("cube-65", "cube", [IDENTITY, GENERIC2, SIDE], 64.0),        # faces of 65 x 65 pixels
    ("cube-2000", "cube", [IDENTITY], 2000.0),
    ("tetrahedron", "tetrahedron", [IDENTITY, GENERIC, GENERIC2], 23.7),
    ("triangle-none", "triangle", [IDENTITY], 0.4),               # covers no centre
    ("triangle-one", "triangle", [IDENTITY], 1.3),                # covers the centre (0.5, 0.5) alone
    ("triangle-257x3", "triangle", [STRETCH_257, STRETCH_256], 1.0),
    ("open_square", "open_square", [IDENTITY, GENERIC, SIDE], 31.5),
    ("l_prism", "l_prism", [IDENTITY, GENERIC, GENERIC2, SIDE], 20.3),
    ("occluded_cubes", "occluded_cubes", [IDENTITY, GENERIC], 40.0),
    ("icosphere", "icosphere", [IDENTITY, GENERIC, GENERIC2], 16.0),
    ("icosphere-small", "icosphere", [GENERIC], 3.1),             # most faces below a pixel
    ("roof", "roof", [GRAZING, IDENTITY, GENERIC], 60.0),
    ("degenerate", "degenerate", [IDENTITY, GENERIC], 12.5),
    ("icosphere3_bumped", "icosphere3_bumped", [GENERIC, GENERIC2, IDENTITY], 33.7),   # 3 vertex, 80 face and 8 edge blocks a view
    ("fence", "fence", [IDENTITY], 8.0),                          # 41 lines on each long edge, a box 969 pixels wide
    ("fence-turned", "fence", [FENCE_TURNED], 7.3),               # (a case has one scale: the fence's two views are two cases)
    ("triangle-3x257", "triangle", [TALL_257, TALL_256], 1.0),
]


def case(name):
    for n, mesh, views, scale in CASES:
        if n == name:
            v, f = MESHES[mesh]()
            return v, f, np.stack(views), np.float32(scale)
    raise KeyError(name)
