"""The referee of "Templates from a mesh: exact visibility and joined lines" (include/fdcm.h), on top of tests/mesh_ref.py: the
exact visibility rule (A) as brute force over all faces, and the joining of a view's runs into chains and their greedy
simplification (B), in numpy float32 (one rounding per operation, in the order written there) and Python integers.  Nothing
here comes from the kernels: no tiles, no link table -- the chains are found by following dictionaries."""
import numpy as np

import mesh_ref as MR

F32 = np.float32
MAX_SPAN_SEGMENTS = 256
ITEMS, EXACT = "items", "exact"


def exact_visibility(mesh, X, Y, Z, e, depth_tol):
    """The visibility of the samples of edge e under rule A, and the samples (SX, SY): every face is tried."""
    A, B = (int(i) for i in mesh.everts[e])
    with np.errstate(all="ignore"):
        dx, dy, dz = X[B] - X[A], Y[B] - Y[A], Z[B] - Z[A]
        n = max(1, int(np.ceil(max(abs(dx), abs(dy)))))
        t = np.arange(n + 1).astype(np.float32) / F32(n)
        SX, SY, SZ = X[A] + t * dx, Y[A] + t * dy, Z[A] + t * dz
        limit = SZ + F32(depth_tol)
    # all faces at once: arrays (F, n + 1), every operation the float32 one of the scalar statement
    a, b, c = mesh.f[:, 0], mesh.f[:, 1], mesh.f[:, 2]
    col = lambda w, i: w[i][:, None]
    px, py = SX[None, :], SY[None, :]
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
        hides = covers & (zf > limit[None, :])          # (False for a NaN zf)
    own = np.arange(len(mesh.f))
    hides[(own == mesh.efaces[e, 0]) | (own == mesh.efaces[e, 1])] = False
    hides[(mesh.f == A).any(axis=1), 0] = False
    hides[(mesh.f == B).any(axis=1), n] = False
    return ~hides.any(axis=0), SX, SY


def edge_runs(mesh, X, Y, Z, box, D, e, depth_tol, visibility):
    """(runs [(k0, k1)], SX, SY, vis) of candidate edge e: the maximal runs k0 < k1 of visible samples, by either rule."""
    if visibility == EXACT:
        vis, SX, SY = exact_visibility(mesh, X, Y, Z, e, depth_tol)
    else:
        vis = MR.edge_lines(mesh, X, Y, Z, box, D, e, depth_tol, 0.0)[1]
        A, B = mesh.everts[e]
        with np.errstate(all="ignore"):
            dx, dy = X[B] - X[A], Y[B] - Y[A]
            n = max(1, int(np.ceil(max(abs(dx), abs(dy)))))
            t = np.arange(n + 1).astype(np.float32) / F32(n)
            SX, SY = X[A] + t * dx, Y[A] + t * dy
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
    return runs, SX, SY, vis


def _length(x0, y0, x1, y1):
    with np.errstate(all="ignore"):
        ddx, ddy = x1 - x0, y1 - y0
        return np.sqrt(ddx * ddx + ddy * ddy)


def simplify(P, tol):
    """The greedy simplification of the chain points P (a list of (x, y) float32): the emitted lines (x0, y0, x1, y1)."""
    return [(P[a][0], P[a][1], P[j][0], P[j][1]) for a, j in simplify_spans(P, tol)]


def simplify_spans(P, tol):
    """The emitted lines as pairs of indices (a, j) into P."""
    tt = F32(tol) * F32(tol)
    m = len(P) - 1
    out, a = [], 0
    for j in range(2, m + 1):
        with np.errstate(all="ignore"):
            dx, dy = P[j][0] - P[a][0], P[j][1] - P[a][1]
            L2 = dx * dx + dy * dy
            ok = bool(L2 > 0) and j - a <= MAX_SPAN_SEGMENTS
            i = a + 1
            while ok and i < j:
                wx, wy = P[i][0] - P[a][0], P[i][1] - P[a][1]
                s = dx * wx + dy * wy
                c = dx * wy - dy * wx
                ok = bool(0 <= s) and bool(s <= L2) and bool(c * c <= tt * L2)
                i += 1
        if not ok:
            out.append((a, j - 1))
            a = j - 1
    out.append((a, m))
    return out


def chains(pre):
    """pre: the view's lines before joining, dicts with `ends`: [(vertex or None, point), (vertex or None, point)] for the start
    and the finish end.  Returns the chains in order, each a list of (line, entered end)."""
    at = {}
    for i, ln in enumerate(pre):
        for end in (0, 1):
            v = ln["ends"][end][0]
            if v is not None:
                at.setdefault(v, []).append((i, end))
    link = {}
    for ends in at.values():
        if len(ends) == 2:
            link[ends[0]], link[ends[1]] = ends[1], ends[0]
    seen, out = set(), []
    for i in range(len(pre)):
        if i in seen:
            continue
        # the chain of line i: walk back from its start end to a free end, or once round
        line, end, cyc = i, 0, False
        while (line, end) in link:
            line, end = link[(line, end)]
            end = 1 - end                       # the end we would leave that line by, walking backwards
            if line == i:
                cyc = True
                break
        if cyc:
            members = [(i, 0)]
            line, end = i, 1
            while link[(line, end)][0] != i:
                line, e_in = link[(line, end)]
                members.append((line, e_in))
                end = 1 - e_in
            # a cycle starts with its lowest line, entered at its start end
            assert min(l for l, _ in members) == i
            if members[0][1] != 0:
                raise AssertionError("cycle walk")
        else:
            # (line, end) is a free end: walk forward from it
            first = (line, end)
            members = [first]
            cl, ce = first
            while (cl, 1 - ce) in link:
                cl, ce = link[(cl, 1 - ce)]
                members.append((cl, ce))
            if members[-1][0] < members[0][0]:  # the path starts at the free end of the lower-indexed end line
                members = [(l, 1 - en) for l, en in reversed(members)]
        seen.update(l for l, _ in members)
        out.append(members)
    out.sort(key=lambda ch: ch[0][0])
    return out


def view_lines(mesh, R, scale, depth_tol, min_length, visibility=ITEMS, join_tolerance=None, want_chains=False):
    """(N, 4) float32 lines of one view; None where the view is refused.  want_chains: (lines, info, pre), info per chain
    its (line, entered end) members, its points and its emitted lines before the length test."""
    if visibility not in (ITEMS, EXACT):
        raise ValueError("visibility")
    if join_tolerance is not None and not (np.isfinite(join_tolerance)):
        raise ValueError("join_tolerance")
    runs = view_runs(mesh, R, scale, depth_tol, visibility)
    if runs is None:
        return None
    return lines_of_runs(runs, min_length, join_tolerance, want_chains)


def view_runs(mesh, R, scale, depth_tol, visibility):
    """The runs of one view, which depend on neither min_length nor the joining: a list of (line x0 y0 x1 y1, its length, ends
    [(vertex or None, point)] * 2) in (edge, k0) order, the lengths > 0; None where the view is refused."""
    X, Y, Z = MR.project(mesh.v, R, scale)
    box = MR.view_box(X, Y)
    if box is None:
        return None
    D = MR.item_buffer(mesh, X, Y, Z, box) if visibility == ITEMS else None
    out = []
    for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
        runs, SX, SY, _ = edge_runs(mesh, X, Y, Z, box, D, e, depth_tol, visibility)
        n = len(SX) - 1
        A, B = (int(i) for i in mesh.everts[e])
        for k0, k1 in runs:
            length = _length(SX[k0], SY[k0], SX[k1], SY[k1])
            if not length > 0:
                continue
            start = (A, (X[A], Y[A])) if k0 == 0 else (None, (SX[k0], SY[k0]))
            finish = (B, (X[B], Y[B])) if k1 == n else (None, (SX[k1], SY[k1]))
            out.append(((SX[k0], SY[k0], SX[k1], SY[k1]), length, [start, finish], int(e)))
    return out


def lines_of_runs(runs, min_length, join_tolerance=None, want_chains=False):
    """The lines of view_runs' result: the length test alone, or joined first."""
    join = join_tolerance is not None and join_tolerance >= 0
    if not join:
        out = [ln for ln, length, _, _ in runs if length >= F32(min_length)]
        lines = np.array(out, dtype=np.float32).reshape(-1, 4)
        return (lines, [], []) if want_chains else lines
    pre = [{"edge": e, "ends": ends} for _, _, ends, e in runs]
    out, info = [], []
    for members in chains(pre):
        l0, e0 = members[0]
        P = [pre[l0]["ends"][e0][1]] + [pre[l]["ends"][1 - en][1] for l, en in members]
        emitted = simplify(P, join_tolerance)
        info.append((members, P, emitted))
        for ln in emitted:
            length = _length(*ln)
            if length > 0 and length >= F32(min_length):
                out.append(ln)
    lines = np.array(out, dtype=np.float32).reshape(-1, 4)
    return (lines, info, pre) if want_chains else lines


def views_lines(mesh, views, scale, depth_tol, min_length, visibility=ITEMS, join_tolerance=None):
    """(lines (N, 4) float32, offsets int64 of n_views + 1): every view on its own, one after another."""
    parts = [view_lines(mesh, R, scale, depth_tol, min_length, visibility, join_tolerance)
             for R in np.asarray(views, dtype=np.float32).reshape(-1, 3, 3)]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return (np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)).reshape(-1, 4), offsets
