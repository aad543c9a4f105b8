"""GPU tests of the gate inside the minimum (include/fdcm.h, "Gate inside the minimum").  The referee is the numpy statement
gate_ref.py on planes that never come from a gated or a capped kernel: the uncapped cost maps of the lines (the score maps of
one-line templates) and the uncapped score maps, on a stride-1 master grid, computed once.  The case is tools/gate_probe.py's:
an adopted random volume of 4 x 41 x 89, twelve templates of 0 to 17 lines, three rotations (one not of unit norm), strides
(2, 3), caps near the median line cost with some +inf and one 0, min_matched 0.5."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import nms_ref
from capped_ref import capped_volumes, line_cost_maps
from detect_all_ref import denominators, detect_all_ref, thresholded
from detect_ref import best_ref, normalised
from gate_ref import gated_best, gated_volumes, of_best, pair_matched_lengths
from matched_ref import gated, matched_lengths, need, totals
from window_detect_ref import detect_windows_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "gate_probe.py")
DEFAULT = 0
f32 = np.float32
INF = float("inf")


def _load():
    spec = importlib.util.spec_from_file_location("gate_probe", PROBE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bytes(got):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in got)


class Planes:
    """What the referee reads for one device map, with rotations (rot) and without: on the master grid the uncapped cost of
    every line, the capped scores (numpy clamp and Eigen-order sum), q and ML of every pair."""

    def __init__(self, w, dev, rot):
        from openfdcm_amd.engine import DeviceTemplates
        self.w, self.dev, self.rot = w, dev, rot
        self.cs, self.piv = (w["cs"], w["piv"]) if rot else (None, None)
        self.A = len(w["cs"]) if rot else 1
        tmpls, caps, lens = w["tmpls"], w["caps"], w["lens"]
        X0, Y0, NX, NY = w["master"]
        mg = (X0, Y0, NX, NY, 1, 1)
        cost, self.off = line_cost_maps(dev, tmpls, mg, self.cs, self.piv)
        self.cost = cost if rot else cost[:, None]  # (L, A, NY, NX)
        plain = DeviceTemplates(tmpls)
        unc = dev.rotation_score_map(plain, mg, self.cs, self.piv) if rot else dev.score_map(plain, mg)[:, None]
        self.score = capped_volumes(self.cost, self.off, caps, unc)  # (T, A, NY, NX)
        self.q = normalised(self.score, w["lengths"], DEFAULT)
        self.ml = pair_matched_lengths(self.cost, self.off, caps, lens)
        for a in (self.cost, self.score, self.q, self.ml):
            a.setflags(write=False)
        self.boxes = nms_ref.footprints(tmpls, self.cs, self.piv, margin=w["probe"].MARGIN)
        self.grid = (dev.exhaustive_rotations_window(w["tset"], self.cs, self.piv, *w["probe"].STRIDE) if rot
                     else dev.exhaustive_window(w["tset"], *w["probe"].STRIDE)).as_tuple()

    def on(self, a, grid):
        """a (.., NY, NX) on the master grid at the points of grid."""
        x0, y0, nx, ny, sx, sy = grid
        X0, Y0, NX, NY = self.w["master"]
        rows, cols = y0 - Y0 + sy * np.arange(ny), x0 - X0 + sx * np.arange(nx)
        assert rows[0] >= 0 and rows[-1] < NY and cols[0] >= 0 and cols[-1] < NX
        return np.ascontiguousarray(a[..., rows, :][..., cols])

    def all_planes(self, mm, grid=None):
        grid = grid or self.grid
        return gated_best(self.on(self.q, grid), self.on(self.ml, grid), mm, self.w["lens"], skip=self.w["skip"])

    def winner_planes(self, mm, grid=None):
        """(scores, pairs) of the existing gate: the unrestricted best map without the points whose pair fails."""
        grid = grid or self.grid
        s0, p0 = best_ref(self.on(self.q, grid), self.w["skip"])
        ml = self.on(self.ml, grid)
        ml = ml.reshape((-1,) + ml.shape[2:])
        return gated(s0, p0, of_best(ml, p0), need(mm, np.repeat(totals(self.w["lens"]), self.A))) + (s0, p0)

    def detect_ref(self, mm, max_score=INF, md=4096, permille=300, grid=None):
        grid = grid or self.grid
        s, p, fr = self.all_planes(mm, grid)
        rec, F = detect_all_ref(s, p, self.boxes.reshape(-1, 4), grid, max_score, md, permille, self.A, self.cs, self.piv)
        sg, pg = thresholded(s, p, max_score)
        g, _, _ = nms_ref.nms_ref(sg, pg, self.boxes.reshape(-1, 4), grid, md, permille)
        return rec, F, fr.reshape(-1)[g], g, p

    def detect(self, mm, max_score=INF, md=4096, permille=300, gate="all", grid=None, tset=None, dev=None):
        return (dev or self.dev).exhaustive_detect_all(tset or self.w["tset"], grid or self.grid, self.cs, self.piv, max_score=max_score,
                                                       max_detections=md, overlap_permille=permille, margin=self.w["probe"].MARGIN,
                                                       penalty=DEFAULT, boxes=True, min_matched=mm, matched=True, gate=gate)

    def windows_ref(self, jobs, mm, gate, max_score=INF, md=4096, permille=300):
        w = self.w
        has = [tm.shape[1] > 0 for tm in w["tmpls"]]
        vols = [self.score[t] if has[t] else None for t in range(len(has))]
        costs = [self.cost[self.off[t]:self.off[t + 1]] if has[t] else None for t in range(len(has))]
        if gate == "all":
            vols, mm = gated_volumes(vols, self.ml, mm, w["lens"]), 0.0
        sx, sy = w["probe"].STRIDE
        return detect_windows_ref(vols, w["master"], jobs, self.cs, self.piv, sx, sy, denominators(w["lengths"], DEFAULT), self.boxes,
                                  max_score, md, permille, mm, costs, w["caps"], w["lens"])

    def windows(self, jobs, mm, gate, max_score=INF, md=4096, permille=300):
        sx, sy = self.w["probe"].STRIDE
        return self.dev.exhaustive_detect_windows(self.w["tset"], jobs, self.cs, self.piv, sx=sx, sy=sy, wrap=True, max_score=max_score,
                                                  max_detections=md, overlap_permille=permille, margin=self.w["probe"].MARGIN,
                                                  penalty=DEFAULT, min_matched=mm, boxes=True, matched=True, job_index=True, gate=gate)


@pytest.fixture(scope="module")
def world():
    from openfdcm_amd.engine import DeviceTemplates, line_lengths
    probe = _load()
    dev, tmpls, caps, cs, piv, jobs = probe.case()
    tset = DeviceTemplates(tmpls, line_caps=caps)
    w = dict(probe=probe, dev=dev, tmpls=tmpls, caps=caps, cs=cs, piv=piv, jobs=jobs, tset=tset, lens=line_lengths(tmpls),
             lengths=tset.lengths(), skip=[t for t, tm in enumerate(tmpls) if tm.shape[1] == 0], mm=probe.MIN_MATCHED)
    assert [tm.shape[1] for tm in tmpls] == [0, 1, 3, 4, 7, 8, 9, 12, 13, 17, 5, 2] and len(cs) == 3
    assert abs(float(np.hypot(*cs[2])) - 0.9) < 1e-6 and any(np.isinf(c).any() for c in caps) and caps[4][2] == 0
    # the master grid: every window of the case, the dense ones and the jobs'
    sx, sy = probe.STRIDE
    gr, gt = dev.exhaustive_rotations_window(tset, cs, piv, sx, sy).as_tuple(), dev.exhaustive_window(tset, sx, sy).as_tuple()
    xs = [g[0] for g in (gr, gt)] + [g[0] + (g[2] - 1) * sx for g in (gr, gt)] + list(jobs[:, 3]) + list(jobs[:, 3] + (jobs[:, 5] - 1) * sx)
    ys = [g[1] for g in (gr, gt)] + [g[1] + (g[3] - 1) * sy for g in (gr, gt)] + list(jobs[:, 4]) + list(jobs[:, 4] + (jobs[:, 6] - 1) * sy)
    w["master"] = (int(min(xs)), int(min(ys)), int(max(xs) - min(xs) + 1), int(max(ys) - min(ys) + 1))
    # more than one 16 x 64 sub-tile in each direction, with partial tiles
    assert gr[2] > 16 and gr[2] % 16 and gr[3] > 64 and gr[3] % 64, gr
    w[True], w[False] = Planes(w, dev, True), Planes(w, dev, False)
    return w


def test_the_inputs_separate_the_gates(world):
    """On the referee's planes alone: points kept by ALL and dropped by WINNER, points kept by both with the same pair, and
    points with a candidate that both drop."""
    for rot in (True, False):
        P = world[rot]
        s, p, fr = P.all_planes(world["mm"])
        sw, pw, s0, p0 = P.winner_planes(world["mm"])
        n = [int(((p >= 0) & (pw < 0)).sum()), int(((p >= 0) & (pw >= 0) & (p == pw)).sum()), int(((p0 >= 0) & (p < 0)).sum())]
        print("rot", rot, "grid", P.grid, "ALL only, both, neither:", n, "of", int((p0 >= 0).sum()))
        assert min(n) >= 1
        assert not ((pw >= 0) & (p != pw)).any()  # a winner that passes is the smallest key among those that pass


def test_1_the_gated_best_map_is_the_referees_planes(world):
    import openfdcm_amd as fd
    for rot in (True, False):
        P = world[rot]
        want = P.all_planes(world["mm"])
        got = P.dev.best_map(world["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=world["mm"], matched=True)
        assert _bytes(got) == _bytes(want) and [a.dtype for a in got] == [np.float32, np.int32, np.float32]
        two = P.dev.best_map(world["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=world["mm"])
        assert len(two) == 2 and _bytes(two) == _bytes(want[:2])
    P = world[False]  # the public call, on the default window
    got = fd.best_score_map(world["dev"], world["tmpls"], stride=world["probe"].STRIDE, penalty=fd.DefaultPenalty(), line_caps=world["caps"],
                            min_matched=world["mm"], return_matched=True)
    assert got[3] == P.grid and _bytes(got[:3]) == _bytes(P.all_planes(world["mm"]))


def _same(got, want):
    rec, F, fr = want[:3]
    assert np.array_equal(got[0]["tmpl_idx"], rec["tmpl_idx"])
    assert got[0]["score"].tobytes() == rec["score"].tobytes() and got[0]["transform"].tobytes() == rec["transform"].tobytes()
    assert np.array_equal(got[1], F) and got[1].dtype == np.int32
    assert got[2].tobytes() == np.asarray(fr, dtype=np.float32).tobytes()


def test_2_gate_all_records_boxes_and_fractions(world):
    for rot in (True, False):
        P = world[rot]
        n_all = len(P.detect_ref(world["mm"], permille=1000)[0])
        for permille in (300, 1000):
            full = P.detect_ref(world["mm"], permille=permille)
            assert len(full[0]) >= 20
            for md in (4096, len(full[0]), len(full[0]) - 7):  # not reached, just reached, reached
                want = P.detect_ref(world["mm"], permille=permille, md=md)
                assert len(want[0]) == min(md, len(full[0]))
                _same(P.detect(world["mm"], permille=permille, md=md), want)
        print("rot", rot, "candidates", n_all, "detections at overlap 0.3", len(P.detect_ref(world["mm"])[0]))


def _c_dense(P, w, mm, gate, max_score=INF, md=4096, permille=300):
    """fdcm_search_exhaustive_detect_all_gated itself, with the kind of gate as a number."""
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import _adopt_matches, _rotations, as_grid
    rot, keep = _rotations(P.cs, P.piv, w["tset"].count) if P.cs is not None else (None, None)
    g = as_grid(P.grid)
    out, n = C.c_void_p(), C.c_int64()
    fp, fr = np.zeros((md, 4), dtype=np.int32), np.zeros(md, dtype=np.float32)
    capi.check(capi.lib().fdcm_search_exhaustive_detect_all_gated(
        P.dev._h, w["tset"]._h, C.byref(rot) if rot is not None else None, C.byref(g), float(max_score), md, permille, w["probe"].MARGIN,
        DEFAULT, 1.0, float(mm), gate, 0, C.byref(out), C.byref(n), fp.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(fr)))
    return _adopt_matches(out, n.value), fp[:n.value].copy(), fr[:n.value].copy()


def _c_windows(P, w, jobs, mm, gate, md=4096, permille=300):
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import _adopt_matches, _rotations, as_pose_windows
    rot, keep = _rotations(P.cs, P.piv, w["tset"].count) if P.cs is not None else (None, None)
    jobs = as_pose_windows(jobs)
    out, n = C.c_void_p(), C.c_int64()
    fp, fr, ji = np.zeros((md, 4), dtype=np.int32), np.zeros(md, dtype=np.float32), np.zeros(md, dtype=np.int32)
    sx, sy = w["probe"].STRIDE
    capi.check(capi.lib().fdcm_search_exhaustive_detect_windows_gated(
        P.dev._h, w["tset"]._h, C.byref(rot) if rot is not None else None, jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)), jobs.shape[0],
        sx, sy, 1, INF, md, permille, w["probe"].MARGIN, DEFAULT, 1.0, float(mm), gate, 0, C.byref(out), C.byref(n),
        fp.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(fr), ji.ctypes.data_as(C.POINTER(C.c_int32))))
    return _adopt_matches(out, n.value), fp[:n.value].copy(), fr[:n.value].copy(), ji[:n.value].copy()


def test_3_gate_winner_and_min_matched_zero_are_the_existing_calls(world):
    w, mm = world, world["mm"]
    for rot in (True, False):
        P = w[rot]
        old = P.detect(mm, gate="winner")  # the existing entry point
        assert len(old[0]) >= 10
        assert _bytes(_c_dense(P, w, mm, 0)) == _bytes(old)
        assert _bytes(_c_dense(P, w, mm, 1)) == _bytes(P.detect(mm, gate="all")) != _bytes(old)
        ungated = P.dev.exhaustive_detect_all(w["tset"], P.grid, P.cs, P.piv, max_detections=4096, overlap_permille=300,
                                              margin=w["probe"].MARGIN, penalty=DEFAULT, boxes=True)
        for gate in (0, 1):
            got = _c_dense(P, w, 0.0, gate)
            assert _bytes(got[:2]) == _bytes(ungated)
        assert _bytes(P.detect(0.0, gate="all")) == _bytes(P.detect(0.0, gate="winner"))
        s0, p0 = P.dev.best_map(w["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT)
        s, p, fr = P.dev.best_map(w["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=0.0, matched=True)
        assert s.tobytes() == s0.tobytes() and p.tobytes() == p0.tobytes() and np.array_equal(np.isnan(fr), p0 < 0)
    P, jobs = w[True], w["jobs"]
    old = P.windows(jobs, mm, "winner")
    assert len(old[0]) >= 10 and _bytes(_c_windows(P, w, jobs, mm, 0)) == _bytes(old)
    assert _bytes(_c_windows(P, w, jobs, mm, 1)) == _bytes(P.windows(jobs, mm, "all"))
    assert _bytes(_c_windows(P, w, jobs, 0.0, 1)) == _bytes(_c_windows(P, w, jobs, 0.0, 0)) == _bytes(P.windows(jobs, None, "winner"))


def test_4_caps_of_infinity_give_the_ungated_bytes(world):
    """A finite volume and no finite cap: every line is matched, every fraction is 1 and no gate removes anything."""
    from openfdcm_amd.engine import DeviceTemplates
    w = world
    open_caps = DeviceTemplates(w["tmpls"], line_caps=[np.full(tm.shape[1], np.inf, dtype=np.float32) for tm in w["tmpls"]])
    for tset in (open_caps, DeviceTemplates(w["tmpls"])):
        for rot in (True, False):
            P = w[rot]
            want = P.detect(None, tset=tset, gate="winner")
            assert len(want[0]) >= 10 and np.all(want[2] == 1)
            for mm in (0.3, 1.0):
                for gate in ("winner", "all"):
                    assert _bytes(P.detect(mm, tset=tset, gate=gate)) == _bytes(want)
            s0, p0 = P.dev.best_map(tset, P.grid, P.cs, P.piv, penalty=DEFAULT)
            s, p = P.dev.best_map(tset, P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=1.0)
            assert s.tobytes() == s0.tobytes() and p.tobytes() == p0.tobytes()


def test_5_every_winner_record_is_a_record_of_gate_all(world):
    for rot in (True, False):
        P = world[rot]
        a, b = P.detect(world["mm"], permille=1000, gate="all"), P.detect(world["mm"], permille=1000, gate="winner")
        assert len(a[0]) < 4096 and len(b[0]) < len(a[0])
        rows = lambda r: {r[0][l].tobytes() + r[1][l].tobytes() + r[2][l].tobytes() for l in range(len(r[0]))}
        assert len(rows(b)) == len(b[0]) and rows(b) < rows(a)


def test_6_fractions_are_matched_fractions_and_pass_the_gate(world):
    from openfdcm_amd.engine import DeviceTemplates
    w = world
    plain = DeviceTemplates(w["tmpls"])
    tl = totals(w["lens"])
    for rot in (True, False):
        P = w[rot]
        rec, F, fr = P.detect(w["mm"], permille=1000)
        want = P.detect_ref(w["mm"], permille=1000)
        g, pairs = want[3], want[4]
        u = pairs.reshape(-1)[g].astype(np.int64)
        x0, y0, nx, ny, sx, sy = P.grid
        poses = np.stack([u // P.A, u % P.A, x0 + (g % nx) * sx, y0 + (g // nx) * sy], axis=1).astype(np.int32)
        assert len(poses) == len(rec) >= 20 and np.array_equal(poses[:, 0], rec["tmpl_idx"])
        assert P.dev.matched_fractions(w["tset"], poses, P.cs, P.piv).tobytes() == fr.tobytes()
        flat, off = P.dev.line_costs(plain, poses, P.cs, P.piv)
        for l, (t, a, x, y) in enumerate(poses):
            ml = matched_lengths(flat[off[l]:off[l + 1]], w["caps"][t], w["lens"][t])
            assert ml >= need(w["mm"], tl[t]) and (f32(ml) / tl[t] if tl[t] else f32(1)) == fr[l]
        assert (fr < 1).any() and (fr >= f32(w["mm"])).all()


def test_7_a_threshold_returns_the_leading_records(world):
    """Three quantiles of the gated plane: the early exit runs, and the records are the +inf list's leading records."""
    for rot in (True, False):
        P = world[rot]
        s = P.all_planes(world["mm"])[0]
        full = P.detect(world["mm"])
        v = np.sort(s[~np.isnan(s)])
        for quant in (0.02, 0.2, 0.6):
            thr = float(v[int(len(v) * quant)])
            got = P.detect(world["mm"], max_score=thr)
            k = int((full[0]["score"] <= f32(thr)).sum())
            assert len(got[0]) == k and _bytes(got) == _bytes(tuple(p[:k] for p in full))
        thr = float(v[int(len(v) * 0.2)])
        want = P.detect_ref(world["mm"], max_score=thr)
        assert 1 <= len(want[0]) < len(full[0])
        _same(P.detect(world["mm"], max_score=thr), want)


def _same_windows(got, want):
    _same(got[:3], want[:3])
    assert np.array_equal(got[3], want[3])


def test_8_windows(world):
    w, jobs, mm = world, world["jobs"], world["mm"]
    P = w[True]
    pts = jobs[:, 2] * jobs[:, 5] * jobs[:, 6]
    assert (pts == 1).sum() >= 10 and pts.max() == 243 and ((jobs[:, 1] + jobs[:, 2]) > 3).sum() >= 5
    assert len({tuple(j) for j in jobs}) < len(jobs) and (jobs[:, 0] == 0).sum() == 2
    every_all, every_win = P.windows_ref(jobs, mm, "all", permille=1000), P.windows_ref(jobs, mm, "winner", permille=1000)
    only = set(every_all[3].tolist()) - set(every_win[3].tolist())
    print("jobs", len(jobs), "ALL", every_all[4], "WINNER", every_win[4], "jobs with a winner under ALL only", sorted(only))
    assert len(only) >= 1 and set(every_win[3].tolist()) <= set(every_all[3].tolist())
    assert every_all[4]["no_winner"] >= 3 and every_all[4]["detections"] >= 20
    thr = float(np.sort(every_all[0]["score"])[len(every_all[0]) // 2])
    for permille, max_score, md in [(1000, INF, 4096), (300, INF, 4096), (300, thr, 4096), (0, INF, 4096), (300, INF, 5)]:
        want = P.windows_ref(jobs, mm, "all", max_score=max_score, md=md, permille=permille)
        _same_windows(P.windows(jobs, mm, "all", max_score=max_score, md=md, permille=permille), want)
        assert len(want[0]) >= 3
    assert (every_all[2] >= f32(mm)).all() and (every_all[2] < 1).any()
    _same_windows(P.windows(jobs, mm, "winner"), P.windows_ref(jobs, mm, "winner"))
    # translations only: a0 = 0, na = 1
    tr = np.array(jobs, dtype=np.int32)
    tr[:, 1], tr[:, 2] = 0, 1
    T = w[False]
    want = T.windows_ref(tr, mm, "all")
    assert len(want[0]) >= 10
    _same_windows(T.windows(tr, mm, "all"), want)


def test_9_refined_is_its_composition(world):
    import openfdcm_amd as fd
    w = world
    coarse, fine = np.array([0.0, 0.3, -0.4]), np.deg2rad(np.arange(-30, 31, 6.0))
    kw = dict(penalty=fd.DefaultPenalty(), line_caps=w["caps"], margin=1)
    seeds = fd.exhaustive_detect_all(w["dev"], w["tmpls"], INF, overlap=1.0, stride=w["probe"].STRIDE, max_detections=48, angles=coarse, **kw)
    jobs = fd.pose_windows(seeds, coarse, fine, fd.template_pivots(w["tmpls"]), 2, 2, 2)
    out = dict(return_boxes=True, return_matched=True, return_jobs=True)
    got, want = {}, {}
    for gate in ("all", "winner"):
        want[gate] = fd.exhaustive_detect_windows(w["dev"], w["tmpls"], jobs, INF, overlap=0.3, angles=fine, min_matched=w["mm"], gate=gate,
                                                  **out, **kw)
        got[gate] = fd.exhaustive_detect_refined(w["dev"], w["tmpls"], INF, coarse, fine, w["probe"].STRIDE, 2, 2, 2,
                                                 coarse_max_detections=48, min_matched=w["mm"], gate=gate, **out, **kw)
        assert len(got[gate]) == 4 and len(got[gate][0]) >= 1
        assert got[gate][0].records().tobytes() == want[gate][0].records().tobytes() and _bytes(got[gate][1:]) == _bytes(want[gate][1:])
    assert _bytes(got["winner"][1:]) == _bytes(fd.exhaustive_detect_refined(
        w["dev"], w["tmpls"], INF, coarse, fine, w["probe"].STRIDE, 2, 2, 2, coarse_max_detections=48, min_matched=w["mm"], **out, **kw)[1:])
    print("refined detections: all", len(got["all"][0]), "winner", len(got["winner"][0]))
    assert len(got["all"][0]) >= len(got["winner"][0])


def _probe(env):
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=300,
                         env={**{k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("gate_probe ")][-1].split()
    return line[1], int(line[3])


def test_10_flat_addresses_give_the_same_bytes(world):
    """In fresh processes (the switches are read once): the 64-bit address forms of the gated kernels."""
    assert not any(k.startswith("FDCM_") for k in os.environ)
    w = world
    dense, win = w["probe"].calls(w["dev"], w["tset"], w["cs"], w["piv"], w["jobs"])
    _same(dense, w[True].detect_ref(w["mm"]))                      # what (2) and (8) hold
    _same_windows(win, w[True].windows_ref(w["jobs"], w["mm"], "all"))
    default = (w["probe"].digest(dense + win), len(dense[0]) + len(win[0]))
    assert default[1] > 40
    assert _probe({"FDCM_MATCHED_FLAT": "1"}) == default
    assert _probe({"FDCM_WINDOWS_FLAT": "1"}) == default


def test_11_the_same_call_twice_and_after_other_calls(world):
    w, mm = world, world["mm"]
    P = w[True]
    first = _bytes(P.detect(mm, max_score=3.0)), _bytes(P.windows(w["jobs"], mm, "all")), _bytes(
        P.dev.best_map(w["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=mm, matched=True))
    P.dev.exhaustive_detect_all(w["tset"], (-20, -20, 70, 90, 1, 1), None, None, max_detections=64, boxes=True)
    again = _bytes(P.detect(mm, max_score=3.0)), _bytes(P.windows(w["jobs"], mm, "all")), _bytes(
        P.dev.best_map(w["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=mm, matched=True))
    assert first == again


def test_a_volume_with_a_nan_and_an_infinity(world):
    """The same case on the volume with one NaN and one +inf planted: planes and records by the referee."""
    w = world
    dev = w["probe"].build(plant=True)
    P = Planes(w, dev, True)
    assert np.isnan(P.cost).sum() > np.isnan(w[True].cost).sum() and np.isinf(P.cost).any()
    want = P.all_planes(w["mm"])
    got = dev.best_map(w["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=w["mm"], matched=True)
    assert _bytes(got) == _bytes(want) and _bytes(want) != _bytes(w[True].all_planes(w["mm"]))
    _same(P.detect(w["mm"], dev=dev), P.detect_ref(w["mm"]))
    _same_windows(P.windows(w["jobs"], w["mm"], "all"), P.windows_ref(w["jobs"], w["mm"], "all"))


def test_empty_inputs_and_a_bad_gate_on_a_device(world):
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = world
    P = w[True]
    none = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for dev, tset in [(none, w["tset"]), (w["dev"], DeviceTemplates([]))]:
        piv = P.piv if tset is w["tset"] else None
        got = dev.exhaustive_detect_all(tset, (0, 0, 5, 5, 1, 1), P.cs, piv, boxes=True, min_matched=0.5, matched=True, gate="all")
        assert [len(p) for p in got] == [0, 0, 0]
        got = dev.exhaustive_detect_windows(tset, w["jobs"][:9], P.cs, piv, wrap=True, min_matched=0.5, boxes=True, matched=True,
                                            job_index=True, gate="all")
        assert [len(p) for p in got] == [0, 0, 0, 0]
        s, p, fr = dev.best_map(tset, (0, 0, 5, 4, 1, 1), P.cs, piv, min_matched=0.5, matched=True)
        assert np.isnan(s).all() and (p == -1).all() and np.isnan(fr).all() and fr.shape == (4, 5)
    got = w["dev"].exhaustive_detect_windows(w["tset"], np.zeros((0, 7), np.int32), P.cs, P.piv, min_matched=0.5, boxes=True, gate="all")
    assert [len(p) for p in got] == [0, 0]
    with pytest.raises(ValueError):
        P.detect(0.5, gate="both")
    _same(P.detect(w["mm"]), P.detect_ref(w["mm"]))  # and a valid call afterwards
