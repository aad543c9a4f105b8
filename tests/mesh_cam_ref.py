"""The referee of "Templates from a mesh: pinhole views" (include/fdcm.h), on top of tests/mesh_ref.py and
tests/mesh_join_ref.py: the pinhole projection, the refusal of a vertex nearer than `near`, and the two depth-tolerance compares
on Z = 1 / depth, in numpy float32 (one rounding per operation, in the order written there).  The pixel box, the item buffer,
the candidates, the runs' lengths, the chains and their simplification are the other two referees' own functions, given this
file's X, Y, Z.  Nothing here comes from the kernels."""
import numpy as np

import mesh_join_ref as JR
import mesh_ref as MR

F32 = np.float32
ITEMS, EXACT = JR.ITEMS, JR.EXACT


def project(v, R, t, focal):
    """(X, Y, Z, d) of the vertices: P.c = ((r_c0 x + r_c1 y) + r_c2 z) + t.c, d = -P.z, Z = 1 / d, X = (focal * P.x) * Z - O.x
    with O.x = (focal * t.x) * (1 / (-t.z)), and Y likewise."""
    R = np.asarray(R, dtype=np.float32).reshape(3, 3)
    t = np.asarray(t, dtype=np.float32).reshape(3)
    f = F32(focal)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        P = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
        d = -P[2]
        Z = F32(1.0) / d
        zo = F32(1.0) / (-t[2])
        ox, oy = (f * t[0]) * zo, (f * t[1]) * zo
        X = (f * P[0]) * Z - ox
        Y = (f * P[1]) * Z - oy
    return X, Y, Z, d


def admitted(d, near):
    """Every vertex has d >= near (a NaN d does not)."""
    return bool(np.all(d >= F32(near)))


def _samples(X, Y, Z, A, B):
    with np.errstate(all="ignore"):
        dx, dy, dz = X[B] - X[A], Y[B] - Y[A], Z[B] - Z[A]
        n = max(1, int(np.ceil(max(abs(dx), abs(dy)))))
        t = np.arange(n + 1).astype(np.float32) / F32(n)
        return X[A] + t * dx, Y[A] + t * dy, Z[A] + t * dz, n


def items_visibility(mesh, X, Y, Z, box, D, e, depth_tol):
    """The item buffer's rule: a judged sample is visible iff (depth_tol * S.Z) * zf >= zf - S.Z."""
    A, B = (int(i) for i in mesh.everts[e])
    x0, y0, x1, y1 = box
    SX, SY, SZ, n = _samples(X, Y, Z, A, B)
    px, py = np.floor(SX).astype(np.int64), np.floor(SY).astype(np.int64)
    vis = np.ones(n + 1, dtype=bool)
    inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
    keys = np.zeros(n + 1, dtype=np.uint64)
    keys[inside] = D[py[inside] - y0, px[inside] - x0]
    owner = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    judged = (keys != 0) & (owner != mesh.efaces[e, 0]) & (owner != mesh.efaces[e, 1])
    for f in np.unique(owner[judged]).tolist():
        at = judged & (owner == f)
        _, zf = MR._depth(X, Y, Z, mesh.f[f].tolist(), SX[at], SY[at])
        with np.errstate(all="ignore"):
            vis[at] = (F32(depth_tol) * SZ[at]) * zf >= zf - SZ[at]
    return vis, SX, SY


def exact_visibility(mesh, X, Y, Z, e, depth_tol):
    """The exact rule, brute force over all faces: hidden iff some admissible covering face has zf - S.Z > (depth_tol * S.Z) * zf."""
    A, B = (int(i) for i in mesh.everts[e])
    SX, SY, SZ, n = _samples(X, Y, Z, A, B)
    a, b, c = mesh.f[:, 0], mesh.f[:, 1], mesh.f[:, 2]
    col = lambda w, i: w[i][:, None]
    px, py, pz = SX[None, :], SY[None, :], SZ[None, :]
    with np.errstate(all="ignore"):
        area = MR._orient(col(X, a), col(Y, a), col(X, b), col(Y, b), col(X, c), col(Y, c))
        xs, ys = X[mesh.f], Y[mesh.f]
        inbox = ((px >= xs.min(axis=1)[:, None]) & (px <= xs.max(axis=1)[:, None]) &
                 (py >= ys.min(axis=1)[:, None]) & (py <= ys.max(axis=1)[:, None]))
        e0 = MR._orient(col(X, b), col(Y, b), col(X, c), col(Y, c), px, py)
        e1 = MR._orient(col(X, c), col(Y, c), col(X, a), col(Y, a), px, py)
        e2 = MR._orient(col(X, a), col(Y, a), col(X, b), col(Y, b), px, py)
        zf = ((e0 * col(Z, a) + e1 * col(Z, b)) + e2 * col(Z, c)) / area
        covers = inbox & ((area > 0) | (area < 0)) & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)))
        hides = covers & (zf - pz > (F32(depth_tol) * pz) * zf)          # (False for a NaN)
    own = np.arange(len(mesh.f))
    hides[(own == mesh.efaces[e, 0]) | (own == mesh.efaces[e, 1])] = False
    hides[(mesh.f == A).any(axis=1), 0] = False
    hides[(mesh.f == B).any(axis=1), n] = False
    return ~hides.any(axis=0), SX, SY


def _runs(vis):
    n = len(vis) - 1
    runs, k = [], 0
    while k <= n:
        if not vis[k]:
            k += 1
            continue
        k1 = k
        while k1 + 1 <= n and vis[k1 + 1]:
            k1 += 1
        if k1 > k:
            runs.append((k, k1))
        k = k1 + 1
    return runs


def view_runs(mesh, R, t, focal, near, depth_tol, visibility, want=False):
    """The runs of one view in the form of mesh_join_ref.view_runs (what lines_of_runs takes); None where the view is refused.
    want: (runs, box, D, (X, Y, Z), per candidate edge its visibility)."""
    X, Y, Z, d = project(mesh.v, R, t, focal)
    if not admitted(d, near):
        return None
    box = MR.view_box(X, Y)
    if box is None:
        return None
    D = MR.item_buffer(mesh, X, Y, Z, box) if visibility == ITEMS or want else None
    out, seen = [], {}
    for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
        if visibility == EXACT:
            vis, SX, SY = exact_visibility(mesh, X, Y, Z, e, depth_tol)
        else:
            vis, SX, SY = items_visibility(mesh, X, Y, Z, box, D, e, depth_tol)
        seen[int(e)] = vis
        n = len(SX) - 1
        A, B = (int(i) for i in mesh.everts[e])
        for k0, k1 in _runs(vis):
            length = JR._length(SX[k0], SY[k0], SX[k1], SY[k1])
            if not length > 0:
                continue
            start = (A, (X[A], Y[A])) if k0 == 0 else (None, (SX[k0], SY[k0]))
            finish = (B, (X[B], Y[B])) if k1 == n else (None, (SX[k1], SY[k1]))
            out.append(((SX[k0], SY[k0], SX[k1], SY[k1]), length, [start, finish], int(e)))
    return (out, box, D, (X, Y, Z), seen) if want else out


def view_lines(mesh, R, t, focal, near, depth_tol, min_length, visibility=ITEMS, join_tolerance=None):
    """(N, 4) float32 lines of one view; None where the view is refused."""
    runs = view_runs(mesh, R, t, focal, near, depth_tol, visibility)
    return None if runs is None else JR.lines_of_runs(runs, min_length, join_tolerance)


def default_near(vertices):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    d = v.max(axis=0) - v.min(axis=0)
    return F32(1e-3 * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
