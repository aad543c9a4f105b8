"""The referee of "Templates from a mesh" (include/fdcm.h): the edge table, the sharp flags, a view's projection, its pixel box
and item buffer, the candidate edges, their samples and the lines, written from the header's definitions in numpy float32 (one
rounding per operation, in the order written there) and Python integers.  Nothing here comes from the kernels; the GPU tests
hold the library to these bytes, and tests/test_mesh_definition.py holds this file to geometry that does not come from it."""
import numpy as np

F32 = np.float32
MAX_SPAN = 4096


class NonManifold(ValueError):
    pass


def edge_table(faces):
    """(verts (E, 2), faces (E, 2) with -1, opposite (E, 2) with -1): the undirected pairs i < j of every face, ascending; a
    pair is counted once per face; the opposite vertex of a face is the index at the position the pair leaves out."""
    inc = {}
    for f, tri in enumerate(np.asarray(faces).tolist()):
        seen = set()
        for k in range(3):
            a, b, c = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
            if a == b:
                continue
            key = (min(a, b), max(a, b))
            if key in seen:
                continue
            seen.add(key)
            inc.setdefault(key, []).append((f, c))
    keys = sorted(inc)
    E = len(keys)
    verts = np.array(keys, dtype=np.int32).reshape(E, 2)
    fa = np.full((E, 2), -1, dtype=np.int32)
    opp = np.full((E, 2), -1, dtype=np.int32)
    for e, key in enumerate(keys):
        lst = sorted(inc[key])
        if len(lst) > 2:
            raise NonManifold(f"non-manifold edge {key}")
        for s, (f, c) in enumerate(lst):
            fa[e, s], opp[e, s] = f, c
    return verts, fa, opp


def _normal(v, tri):
    p0, p1, p2 = (v[i].astype(np.float64) for i in tri)
    u, w = p1 - p0, p2 - p0
    return np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sharp_flags(vertices, faces, efaces, crease_cos):
    v = np.asarray(vertices, dtype=np.float32)
    out = np.zeros(len(efaces), dtype=np.uint8)
    for e, (f0, f1) in enumerate(efaces.tolist()):
        if f1 < 0:
            out[e] = 1
            continue
        n0, n1 = _normal(v, faces[f0]), _normal(v, faces[f1])
        if not n0.any() or not n1.any():
            out[e] = 1
            continue
        out[e] = abs(_dot(n0, n1)) < (float(crease_cos) * np.sqrt(_dot(n0, n0))) * np.sqrt(_dot(n1, n1))
    return out


class Mesh:
    def __init__(self, vertices, faces, crease_cos):
        self.v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self.everts, self.efaces, self.eopp = edge_table(self.f)
        self.sharp = sharp_flags(self.v, self.f, self.efaces, crease_cos)


def project(v, R, scale):
    R = np.asarray(R, dtype=np.float32).reshape(3, 3)
    s = F32(scale)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        P = [(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3)]
        return s * P[0], s * P[1], P[2]


def view_box(X, Y):
    """(x0, y0, x1, y1): floor of the vertices' least and largest X and Y; None where the view is refused."""
    if not (np.all(np.abs(X) < F32(2.0 ** 30)) and np.all(np.abs(Y) < F32(2.0 ** 30))):
        return None
    fx, fy = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    box = (int(fx.min()), int(fy.min()), int(fx.max()), int(fy.max()))
    if box[2] - box[0] + 1 > MAX_SPAN or box[3] - box[1] + 1 > MAX_SPAN:
        return None
    return box


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def ordered(z):
    u = np.asarray(z, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def _depth(X, Y, Z, tri, px, py):
    """(covers?, z) of face tri at the points (px, py), float32 arrays: the header's e0, e1, e2, a and z."""
    A, B, C = tri
    with np.errstate(all="ignore"):
        a = _orient(X[A], Y[A], X[B], Y[B], X[C], Y[C])
        e0 = _orient(X[B], Y[B], X[C], Y[C], px, py)
        e1 = _orient(X[C], Y[C], X[A], Y[A], px, py)
        e2 = _orient(X[A], Y[A], X[B], Y[B], px, py)
        z = ((e0 * Z[A] + e1 * Z[B]) + e2 * Z[C]) / a
    if a > 0:
        inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    elif a < 0:
        inside = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
    else:
        inside = np.zeros(np.shape(e0), dtype=bool)
    return inside & ~np.isnan(z), z


def item_buffer(mesh, X, Y, Z, box):
    """D over the view's box, [row j - y0][column i - x0], uint64: a face is tried at the centres of its own pixel box."""
    x0, y0, x1, y1 = box
    D = np.zeros((y1 - y0 + 1, x1 - x0 + 1), dtype=np.uint64)
    for f, tri in enumerate(mesh.f.tolist()):
        xs, ys = X[tri], Y[tri]
        i0, i1 = int(np.floor(xs.min())), int(np.floor(xs.max()))
        j0, j1 = int(np.floor(ys.min())), int(np.floor(ys.max()))
        cx = (np.arange(i0, i1 + 1).astype(np.float32) + F32(0.5))[None, :]
        cy = (np.arange(j0, j1 + 1).astype(np.float32) + F32(0.5))[:, None]
        inside, z = _depth(X, Y, Z, tri, cx, cy)
        if not inside.any():
            continue
        key = (ordered(z) << np.uint64(32)) | np.uint64(f)
        sub = D[j0 - y0:j1 - y0 + 1, i0 - x0:i1 - x0 + 1]
        np.maximum(sub, np.where(inside, key, np.uint64(0)), out=sub)
    return D


def candidates(mesh, X, Y):
    out = np.zeros(len(mesh.everts), dtype=bool)
    for e in range(len(out)):
        if mesh.sharp[e]:
            out[e] = True
            continue
        A, B = mesh.everts[e]
        with np.errstate(all="ignore"):
            o0 = _orient(X[A], Y[A], X[B], Y[B], X[mesh.eopp[e, 0]], Y[mesh.eopp[e, 0]])
            o1 = _orient(X[A], Y[A], X[B], Y[B], X[mesh.eopp[e, 1]], Y[mesh.eopp[e, 1]])
        out[e] = not ((o0 > 0 and o1 < 0) or (o0 < 0 and o1 > 0))
    return out


def edge_lines(mesh, X, Y, Z, box, D, e, depth_tol, min_length):
    """The kept lines of candidate edge e, in order of k0, and the visibility of its samples."""
    A, B = mesh.everts[e]
    x0, y0, x1, y1 = box
    with np.errstate(all="ignore"):
        dx, dy, dz = X[B] - X[A], Y[B] - Y[A], Z[B] - Z[A]
        n = max(1, int(np.ceil(max(abs(dx), abs(dy)))))
        t = np.arange(n + 1).astype(np.float32) / F32(n)
        SX, SY, SZ = X[A] + t * dx, Y[A] + t * dy, Z[A] + t * dz
    px, py = np.floor(SX).astype(np.int64), np.floor(SY).astype(np.int64)
    vis = np.ones(n + 1, dtype=bool)
    inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
    keys = np.zeros(n + 1, dtype=np.uint64)
    keys[inside] = D[py[inside] - y0, px[inside] - x0]
    owner = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    judged = (keys != 0) & (owner != mesh.efaces[e, 0]) & (owner != mesh.efaces[e, 1])
    for f in np.unique(owner[judged]).tolist():      # the occluder's plane at the samples themselves
        at = judged & (owner == f)
        _, zf = _depth(X, Y, Z, mesh.f[f].tolist(), SX[at], SY[at])
        with np.errstate(all="ignore"):
            vis[at] = SZ[at] + F32(depth_tol) >= zf
    lines = []
    k = 0
    while k <= n:
        if not vis[k]:
            k += 1
            continue
        k1 = k
        while k1 + 1 <= n and vis[k1 + 1]:
            k1 += 1
        if k1 > k:
            with np.errstate(all="ignore"):
                ddx, ddy = SX[k1] - SX[k], SY[k1] - SY[k]
                length = np.sqrt(ddx * ddx + ddy * ddy)
            if length > 0 and length >= F32(min_length):
                lines.append((SX[k], SY[k], SX[k1], SY[k1]))
        k = k1 + 1
    return lines, vis


def view_lines(mesh, R, scale, depth_tol, min_length, want_items=False):
    """(N, 4) float32 lines of one view in (edge, k0) order; None where the view is refused.  want_items: (lines, box, D)."""
    X, Y, Z = project(mesh.v, R, scale)
    box = view_box(X, Y)
    if box is None:
        return None
    D = item_buffer(mesh, X, Y, Z, box)
    cand = candidates(mesh, X, Y)
    out = []
    for e in np.nonzero(cand)[0]:
        out += edge_lines(mesh, X, Y, Z, box, D, e, depth_tol, min_length)[0]
    lines = np.array(out, dtype=np.float32).reshape(-1, 4)
    return (lines, box, D) if want_items else lines


def views_lines(mesh, views, scale, depth_tol, min_length):
    """(lines (N, 4) float32, offsets int64 of n_views + 1): every view on its own, one after another."""
    parts = [view_lines(mesh, R, scale, depth_tol, min_length) for R in np.asarray(views, dtype=np.float32).reshape(-1, 3, 3)]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return (np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)).reshape(-1, 4), offsets


def default_depth_tol(vertices):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    d = v.max(axis=0) - v.min(axis=0)
    return F32(1e-4 * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
