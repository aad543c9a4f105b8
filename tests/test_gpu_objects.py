"""GPU tests of the detector with objects (include/fdcm.h, "Objects").  The referee is the numpy statement objects_ref.py on
planes that come from no object kernel: the uncapped cost maps of the lines and the uncapped score maps on a stride-1 master
grid, as test_gpu_gate.Planes builds them, computed once.  The case is tools/gate_probe.py's (an adopted random volume of
4 x 41 x 89, twelve templates of 0 to 17 lines, three rotations of which one scales, strides (2, 3), caps near the median line
cost) with the labels of tools/objects_probe.py: five objects, object 3 empty, object 4 only the template without lines, no
object's templates contiguous; min_matched (0, 0.5, 0.3, 0.5, 0) and a threshold per object from quantiles of the referee's
planes.  The identities of the header are checked against the existing calls on the device."""
import importlib.util
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from gate_ref import gated_volumes, of_best
from matched_ref import fractions, matched_lengths, need, totals
from objects_ref import detect_objects_ref, objects_best, objects_winner, windows_objects_ref
from detect_all_ref import denominators
from test_gpu_gate import Planes, _bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "objects_probe.py")
DEFAULT = 0
f32 = np.float32
INF = float("inf")
MD = 4096


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def world():
    from openfdcm_amd.engine import DeviceTemplates, line_lengths
    op = _load(PROBE, "objects_probe")
    probe = op.gate_probe()
    dev, tmpls, caps, cs, piv, jobs = probe.case()
    tset = DeviceTemplates(tmpls, line_caps=caps)
    w = dict(probe=probe, op=op, dev=dev, tmpls=tmpls, caps=caps, cs=cs, piv=piv, jobs=jobs, tset=tset, lens=line_lengths(tmpls),
             lengths=tset.lengths(), skip=[t for t, tm in enumerate(tmpls) if tm.shape[1] == 0], mm=probe.MIN_MATCHED,
             obj=np.array(op.OBJECTS, dtype=np.int32), G=op.G, omm=np.float32(op.MIN_MATCHED))
    assert op.OBJECTS == [4, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1] and op.G == 5 and op.MIN_MATCHED == (0.0, 0.5, 0.3, 0.5, 0.0)
    assert w["skip"] == [0] and 3 not in op.OBJECTS  # object 4 holds only the template without lines, object 3 nothing
    sx, sy = probe.STRIDE
    gr, gt = dev.exhaustive_rotations_window(tset, cs, piv, sx, sy).as_tuple(), dev.exhaustive_window(tset, sx, sy).as_tuple()
    xs = [g[0] for g in (gr, gt)] + [g[0] + (g[2] - 1) * sx for g in (gr, gt)] + list(jobs[:, 3]) + list(jobs[:, 3] + (jobs[:, 5] - 1) * sx)
    ys = [g[1] for g in (gr, gt)] + [g[1] + (g[3] - 1) * sy for g in (gr, gt)] + list(jobs[:, 4]) + list(jobs[:, 4] + (jobs[:, 6] - 1) * sy)
    w["master"] = (int(min(xs)), int(min(ys)), int(max(xs) - min(xs) + 1), int(max(ys) - min(ys) + 1))
    assert gr[2] > 16 and gr[2] % 16 and gr[3] > 64 and gr[3] % 64, gr  # several 16 x 64 sub-tiles, partial ones on both axes
    w[True], w[False] = Planes(w, dev, True), Planes(w, dev, False)
    # a threshold per object: the 60 % quantile, the maximum and the 80 % quantile of the object's plane of the referee (gate
    # ALL, rotations).  The entries that only gate ALL keeps lie high in their planes (a pair that passes where the best pair
    # fails has a worse score); object 1, the one with the most of them, keeps all its entries under a finite threshold.
    s = ref_planes(w, w[True], "all")[0]
    ms = np.full(op.G, INF, dtype=np.float32)
    for o, quant in [(0, 0.6), (1, 1.0), (2, 0.8)]:
        v = np.sort(s[o][~np.isnan(s[o])])
        ms[o] = v[min(len(v) - 1, int(len(v) * quant))]
    ms[3], ms[4] = 0.0, 1.0
    w["ms"] = ms
    return w


def ref_planes(w, P, gate, grid=None, obj=None, mm=None):
    """(scores, pairs, fractions), each (G, ny, nx), of the referee under the gate."""
    grid = grid or P.grid
    obj = w["obj"] if obj is None else obj
    mm = w["omm"] if mm is None else mm
    q, ml = P.on(P.q, grid), P.on(P.ml, grid)
    if gate == "all":
        return objects_best(q, ml, obj, len(mm), mm, w["lens"], w["skip"])
    s, p = objects_winner(q, ml, obj, len(mm), mm, w["lens"], w["skip"])
    T, A = q.shape[:2]
    frac = fractions(ml, totals(w["lens"]).reshape(-1, 1, 1, 1)).reshape((T * A,) + q.shape[2:])
    fr = np.stack([of_best(frac, p[o]).astype(np.float32) for o in range(len(mm))])
    fr[p < 0] = np.nan
    return s, p, fr


def ref_detect(w, P, gate, ms=None, md=MD, permille=300, cross=300, obj=None, mm=None):
    ms = w["ms"] if ms is None else ms
    obj = w["obj"] if obj is None else obj
    s, p, fr = ref_planes(w, P, gate, obj=obj, mm=mm)
    return detect_objects_ref(s, p, P.boxes.reshape(-1, 4), P.grid, obj, ms, md, permille, cross, P.A, P.cs, P.piv, fractions=fr)


def detect(w, P, gate, ms=None, md=MD, permille=300, cross=300, obj=None, mm=None, G=None, dev=None):
    ms = w["ms"] if ms is None else ms
    return (dev or P.dev).exhaustive_detect_objects(w["tset"], P.grid, w["obj"] if obj is None else obj, ms, w["G"] if G is None else G,
                                                    P.cs, P.piv, max_detections=md, overlap_permille=permille, cross_permille=cross,
                                                    margin=w["probe"].MARGIN, penalty=DEFAULT, min_matched=w["omm"] if mm is None else mm,
                                                    boxes=True, matched=True, gate=gate)


def windows(w, P, jobs, gate, ms=None, md=MD, permille=300, cross=300, obj=None, mm=None, G=None):
    sx, sy = w["probe"].STRIDE
    ms = w["ms"] if ms is None else ms
    return P.dev.exhaustive_detect_windows_objects(w["tset"], jobs, w["obj"] if obj is None else obj, ms, w["G"] if G is None else G, P.cs,
                                                   P.piv, sx=sx, sy=sy, wrap=True, max_detections=md, overlap_permille=permille,
                                                   cross_permille=cross, margin=w["probe"].MARGIN, penalty=DEFAULT,
                                                   min_matched=w["omm"] if mm is None else mm, boxes=True, matched=True, job_index=True,
                                                   gate=gate)


def _same(got, want):
    rec, F, fr = want[:3]
    assert np.array_equal(got[0]["tmpl_idx"], rec["tmpl_idx"])
    assert got[0]["score"].tobytes() == rec["score"].tobytes() and got[0]["transform"].tobytes() == rec["transform"].tobytes()
    assert np.array_equal(got[1], F) and got[1].dtype == np.int32
    assert got[2].tobytes() == np.asarray(fr, dtype=np.float32).tobytes()


def test_0_the_case_exercises_the_feature(world):
    """On the referee alone, before the device is looked at."""
    w = world
    for rot in (True, False):
        P = w[rot]
        s, p, fr = ref_planes(w, P, "all")
        N = s.shape[1] * s.shape[2]
        several = int(((p >= 0).sum(axis=0) >= 2).sum())
        print("rot", rot, "grid", P.grid, "points with candidates in two or more objects", several, "of", N)
        assert 10 * several >= N
        assert (p[3] < 0).all() and (p[4] < 0).all() and all((p[o] >= 0).any() for o in (0, 1, 2))
        # a detection whose pair is not the single plane's best(g)
        # (the single plane under the same gates: per point the smallest pairkey over the objects' planes)
        pk = np.where(p >= 0, (s.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.maximum(p, 0).astype(np.uint64), np.uint64(2 ** 64 - 1))
        single = np.take_along_axis(p, np.argmin(pk, axis=0)[None], axis=0)[0].reshape(-1)
        lists = {cross: ref_detect(w, P, "all", cross=cross) for cross in (0, 300, 1000)}
        ent = lists[1000][3]
        other = sum(int(p[o].reshape(-1)[g] != single[g]) for o, g in ent)
        print("detections at cross 0 / 300 / 1000:", [len(lists[c][0]) for c in (0, 300, 1000)], "not the single plane's pair:", other)
        assert other >= 1
        assert _bytes(lists[300][:3]) != _bytes(lists[1000][:3]) and _bytes(lists[0][:3]) != _bytes(lists[300][:3])
        wins = {cross: ref_detect(w, P, "winner", cross=cross) for cross in (0, 300, 1000)}
        differ = [cross for cross in (0, 300, 1000) if _bytes(wins[cross][:3]) != _bytes(lists[cross][:3])]
        print("gate WINNER differs from gate ALL at cross", differ)
        assert differ
        every = [ref_detect(w, P, gate, permille=1000, cross=1000) for gate in ("all", "winner")]  # no suppression: every entry
        assert len(every[1][0]) < len(every[0][0]) < MD
        assert all(10 <= len(l[0]) < MD for l in list(lists.values()) + list(wins.values()))
        assert len({o for o, g in ent}) == 3  # every object with candidates is detected


def test_1_the_object_best_map_is_the_referees_planes(world):
    import openfdcm_amd as fd
    w = world
    for rot in (True, False):
        P = w[rot]
        want = ref_planes(w, P, "all")
        got = P.dev.best_map_objects(w["tset"], P.grid, w["obj"], w["G"], P.cs, P.piv, penalty=DEFAULT, min_matched=w["omm"], matched=True)
        assert [a.dtype for a in got] == [np.float32, np.int32, np.float32] and got[0].shape == (5, P.grid[3], P.grid[2])
        assert _bytes(got) == _bytes(want)
        two = P.dev.best_map_objects(w["tset"], P.grid, w["obj"], w["G"], P.cs, P.piv, penalty=DEFAULT, min_matched=w["omm"])
        assert len(two) == 2 and _bytes(two) == _bytes(want[:2])
        # without needs: the planes of the ungated minimum per object
        got = P.dev.best_map_objects(w["tset"], P.grid, w["obj"], w["G"], P.cs, P.piv, penalty=DEFAULT)
        assert _bytes(got) == _bytes(ref_planes(w, P, "all", mm=np.zeros(5, dtype=np.float32))[:2])
    P = w[False]  # the public call, on the default window, n_objects from the labels
    got = fd.object_score_maps(w["dev"], w["tmpls"], w["obj"], stride=w["probe"].STRIDE, penalty=fd.DefaultPenalty(), line_caps=w["caps"],
                               min_matched=w["omm"], return_matched=True)
    assert got[3] == P.grid and _bytes(got[:3]) == _bytes(ref_planes(w, P, "all"))


def test_2_records_boxes_and_fractions_are_the_referees(world):
    w = world
    for rot in (True, False):
        P = w[rot]
        for gate in ("all", "winner"):
            for cross in (0, 300, 1000):
                want = ref_detect(w, P, gate, cross=cross)
                _same(detect(w, P, gate, cross=cross), want)
                assert len(want[0]) >= 10
            full = ref_detect(w, P, gate, cross=300)
            for md in (len(full[0]), len(full[0]) - 7, 1):  # just reached, reached
                want = ref_detect(w, P, gate, cross=300, md=md)
                assert len(want[0]) == md
                _same(detect(w, P, gate, cross=300, md=md), want)
        for gate in ("all", "winner"):  # no suppression: every entry under its threshold, in order
            want = ref_detect(w, P, gate, permille=1000, cross=1000)
            assert len(want[0]) > 500
            _same(detect(w, P, gate, permille=1000, cross=1000), want)
        # no threshold, and limits the other way round
        ms = np.full(5, INF, dtype=np.float32)
        _same(detect(w, P, "all", ms=ms, permille=600, cross=100), ref_detect(w, P, "all", ms=ms, permille=600, cross=100))


def test_3_the_public_call_and_its_objects(world):
    import openfdcm_amd as fd
    w = world
    P = w[False]
    got = fd.exhaustive_detect_objects(w["dev"], w["tmpls"], w["obj"], w["ms"], overlap=0.3, cross_overlap=1.0, stride=w["probe"].STRIDE,
                                       penalty=fd.DefaultPenalty(), line_caps=w["caps"], margin=w["probe"].MARGIN, min_matched=w["omm"],
                                       return_boxes=True, return_matched=True, return_objects=True, gate="all", max_detections=MD)
    want = ref_detect(w, P, "all", cross=1000)
    _same((got[0].records(),) + tuple(got[1:3]), want)
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3][:, 0])
    same = fd.exhaustive_detect_objects(w["dev"], w["tmpls"], w["obj"], w["ms"], stride=w["probe"].STRIDE, penalty=fd.DefaultPenalty(),
                                        line_caps=w["caps"], margin=w["probe"].MARGIN, min_matched=w["omm"], gate="all", max_detections=MD)
    assert same.records().tobytes() == ref_detect(w, P, "all", cross=300)[0].tobytes()  # cross_overlap None: equal to overlap


def _old_dense(w, P, mm, gate, max_score=INF, md=MD, permille=300, tset=None, piv=None):
    return P.dev.exhaustive_detect_all(tset or w["tset"], P.grid, P.cs, P.piv if piv is None else piv, max_score=max_score,
                                       max_detections=md, overlap_permille=permille, margin=w["probe"].MARGIN, penalty=DEFAULT, boxes=True,
                                       min_matched=mm, matched=True, gate=gate)


def test_identity_1_one_object_is_the_existing_calls(world):
    w = world
    one = np.zeros(12, dtype=np.int32)
    sx, sy = w["probe"].STRIDE
    for rot in (True, False):
        P = w[rot]
        thr = float(w["ms"][0])
        for gate in ("all", "winner"):
            for mm, ms in [(0.5, INF), (0.5, thr), (0.0, thr)]:
                old = _old_dense(w, P, mm, gate, max_score=ms)
                assert len(old[0]) >= 5
                for cross in (0, 300, 1000):
                    assert _bytes(detect(w, P, gate, ms=ms, cross=cross, obj=one, mm=mm, G=1)) == _bytes(old)
        old = P.dev.best_map(w["tset"], P.grid, P.cs, P.piv, penalty=DEFAULT, min_matched=0.5, matched=True)
        got = P.dev.best_map_objects(w["tset"], P.grid, one, 1, P.cs, P.piv, penalty=DEFAULT, min_matched=0.5, matched=True)
        assert got[0].shape == (1,) + old[0].shape and _bytes(got) == _bytes(old)
    P = w[True]
    for gate in ("all", "winner"):
        for mm, ms in [(0.5, INF), (0.2, 2.0), (0.0, INF)]:
            old = P.dev.exhaustive_detect_windows(w["tset"], w["jobs"], P.cs, P.piv, sx=sx, sy=sy, wrap=True, max_score=ms, max_detections=MD,
                                                  overlap_permille=300, margin=w["probe"].MARGIN, penalty=DEFAULT, min_matched=mm, boxes=True,
                                                  matched=True, job_index=True, gate=gate)
            assert len(old[0]) >= 5
            for cross in (0, 1000):
                assert _bytes(windows(w, P, w["jobs"], gate, ms=ms, cross=cross, obj=one, mm=mm, G=1)) == _bytes(old)


def _entry_of(P, rec, box):
    """(g, u) of a record of a dense call on P.grid from its template, rotation and footprint."""
    x0, y0, nx, ny, sx, sy = P.grid
    t = int(rec["tmpl_idx"])
    a = 0
    if P.cs is not None:
        hit = np.flatnonzero((P.cs[:, 0] == rec["transform"][0]) & (P.cs[:, 1] == rec["transform"][3]))
        assert len(hit) == 1
        a = int(hit[0])
    b = P.boxes[t, a]
    tx, ty = int(box[0]) - int(b[0]), int(box[1]) - int(b[1])
    i, j = (tx - x0) // sx, (ty - y0) // sy
    assert x0 + i * sx == tx and y0 + j * sy == ty and 0 <= i < nx and 0 <= j < ny
    return j * nx + i, t * P.A + a


def test_identity_2_at_cross_1000_the_objects_do_not_interact(world):
    """The existing dense call once per object on that object's templates, indices mapped back, merged by (score bits, g, u);
    plane o of the object best map is fdcm_best_map_gated of the sub-set."""
    from openfdcm_amd.engine import DeviceTemplates
    w = world
    for rot in (True, False):
        P = w[rot]
        planes = P.dev.best_map_objects(w["tset"], P.grid, w["obj"], w["G"], P.cs, P.piv, penalty=DEFAULT, min_matched=w["omm"], matched=True)
        for gate in ("all", "winner"):
            rows = []
            for o in range(w["G"]):
                idx = [t for t in range(12) if w["obj"][t] == o]
                if not idx:
                    continue
                sub = DeviceTemplates([w["tmpls"][t] for t in idx], line_caps=[w["caps"][t] for t in idx])
                piv = P.piv[idx] if P.piv is not None else None
                rec, box, fr = _old_dense(w, P, float(w["omm"][o]), gate, max_score=float(w["ms"][o]), tset=sub, piv=piv)
                assert len(rec) < MD
                rec = rec.copy()
                rec["tmpl_idx"] = np.array(idx)[rec["tmpl_idx"]]
                for l in range(len(rec)):
                    g, u = _entry_of(P, rec[l], box[l])
                    rows.append(((int(rec["score"][l:l + 1].view(np.uint32)[0]), g, u), rec[l].tobytes(), box[l].tobytes(), fr[l:l + 1].tobytes()))
                if gate == "all":
                    s, p, m = P.dev.best_map(sub, P.grid, P.cs, piv, penalty=DEFAULT, min_matched=float(w["omm"][o]), matched=True)
                    back = np.where(p >= 0, np.array(idx)[np.maximum(p, 0) // P.A] * P.A + p % P.A, -1).astype(np.int32)
                    assert planes[0][o].tobytes() == s.tobytes() and np.array_equal(planes[1][o], back) and planes[2][o].tobytes() == m.tobytes()
            rows.sort(key=lambda r: r[0])
            got = detect(w, P, gate, cross=1000)
            assert len(got[0]) == len(rows) >= 10
            assert got[0].tobytes() == b"".join(r[1] for r in rows) and got[1].tobytes() == b"".join(r[2] for r in rows)
            assert got[2].tobytes() == b"".join(r[3] for r in rows)


def test_identity_3_one_point_windows_of_every_entry_give_the_dense_records(world):
    w = world
    sx, sy = w["probe"].STRIDE
    for rot in (True, False):
        P = w[rot]
        x0, y0, nx, ny = P.grid[:4]
        s, p = P.dev.best_map_objects(w["tset"], P.grid, w["obj"], w["G"], P.cs, P.piv, penalty=DEFAULT, min_matched=w["omm"])
        o, g = np.nonzero(p.reshape(w["G"], -1) >= 0)
        u = p.reshape(w["G"], -1)[o, g].astype(np.int64)
        order = np.lexsort((u, g))
        g, u = g[order], u[order]
        jobs = np.stack([u // P.A, u % P.A, np.ones_like(u), x0 + (g % nx) * sx, y0 + (g // nx) * sy, np.ones_like(u), np.ones_like(u)],
                        axis=1).astype(np.int32)
        assert len(jobs) > nx * ny  # more entries than points
        for cross in (0, 300, 1000):
            dense = detect(w, P, "all", cross=cross)
            win = windows(w, P, jobs, "all", cross=cross)
            assert len(dense[0]) >= 10 and _bytes(win[:3]) == _bytes(dense)
            assert np.array_equal(jobs[win[3], 0], dense[0]["tmpl_idx"])


def test_identity_4_relabelling_changes_no_byte(world):
    w = world
    perm = np.array([3, 0, 4, 1, 2])  # old label -> new label
    inv = np.argsort(perm)
    obj2, ms2, mm2 = perm[w["obj"]].astype(np.int32), w["ms"][inv], w["omm"][inv]
    for rot in (True, False):
        P = w[rot]
        for gate in ("all", "winner"):
            assert _bytes(detect(w, P, gate, cross=600, obj=obj2, ms=ms2, mm=mm2)) == _bytes(detect(w, P, gate, cross=600))
        a = P.dev.best_map_objects(w["tset"], P.grid, w["obj"], 5, P.cs, P.piv, penalty=DEFAULT, min_matched=w["omm"], matched=True)
        b = P.dev.best_map_objects(w["tset"], P.grid, obj2, 5, P.cs, P.piv, penalty=DEFAULT, min_matched=mm2, matched=True)
        assert _bytes([x[inv] for x in a]) == _bytes(b)
    P = w[True]
    assert _bytes(windows(w, P, w["jobs"], "all", cross=600, obj=obj2, ms=ms2, mm=mm2)) == _bytes(windows(w, P, w["jobs"], "all", cross=600))


def test_identity_5_one_threshold_returns_the_leading_records(world):
    w = world
    for rot in (True, False):
        P = w[rot]
        s = ref_planes(w, P, "all")[0]
        v = np.sort(s[~np.isnan(s)])
        full = detect(w, P, "all", ms=INF, cross=600)
        for quant in (0.02, 0.2, 0.6):
            thr = float(v[int(len(v) * quant)])
            got = detect(w, P, "all", ms=thr, cross=600)
            k = int((full[0]["score"] <= f32(thr)).sum())
            assert 0 < k < len(full[0]) and len(got[0]) == k and _bytes(got) == _bytes(tuple(x[:k] for x in full))


def test_identity_6_no_overlap_allowed_means_no_shared_pixel(world):
    w = world
    for rot in (True, False):
        P = w[rot]
        rec, F, fr = detect(w, P, "all", ms=INF, permille=0, cross=0)
        assert len(rec) >= 5
        F = F.astype(np.int64)
        for i in range(len(F)):
            ix = np.minimum(F[i, 2], F[:i, 2]) - np.maximum(F[i, 0], F[:i, 0]) + 1
            iy = np.minimum(F[i, 3], F[:i, 3]) - np.maximum(F[i, 1], F[:i, 1]) + 1
            assert not ((ix > 0) & (iy > 0)).any()


def test_identity_7_fractions_are_matched_fractions_and_pass_the_gate(world):
    from openfdcm_amd.engine import DeviceTemplates
    w = world
    plain = DeviceTemplates(w["tmpls"])
    tl = totals(w["lens"])
    for rot in (True, False):
        P = w[rot]
        for gate in ("all", "winner"):
            rec, F, fr = detect(w, P, gate, cross=1000)
            x0, y0, nx, ny, sx, sy = P.grid
            ent = [_entry_of(P, rec[l], F[l]) for l in range(len(rec))]
            poses = np.array([(u // P.A, u % P.A, x0 + (g % nx) * sx, y0 + (g // nx) * sy) for g, u in ent], dtype=np.int32)
            assert len(poses) >= 20
            assert P.dev.matched_fractions(w["tset"], poses, P.cs, P.piv).tobytes() == fr.tobytes()
            flat, off = P.dev.line_costs(plain, poses, P.cs, P.piv)
            for l, (t, a, x, y) in enumerate(poses):
                ml = matched_lengths(flat[off[l]:off[l + 1]], w["caps"][t], w["lens"][t])
                assert ml >= need(float(w["omm"][w["obj"][t]]), tl[t]) and (f32(ml) / tl[t] if tl[t] else f32(1)) == fr[l]
            assert (fr < 1).any()


def _windows_ref(w, P, jobs, gate, ms=None, md=MD, permille=300, cross=300):
    ms = w["ms"] if ms is None else ms
    has = [tm.shape[1] > 0 for tm in w["tmpls"]]
    vols = [P.score[t] if has[t] else None for t in range(len(has))]
    costs = [P.cost[P.off[t]:P.off[t + 1]] if has[t] else None for t in range(len(has))]
    mm = w["omm"]
    if gate == "all":
        vols, mm = {o: gated_volumes(vols, P.ml, float(w["omm"][o]), w["lens"]) for o in range(w["G"])}, np.zeros(w["G"], dtype=np.float32)
    sx, sy = w["probe"].STRIDE
    return windows_objects_ref(vols, w["master"], jobs, P.cs, P.piv, sx, sy, denominators(w["lengths"], DEFAULT), P.boxes, w["obj"], ms, mm,
                               md, permille, cross, costs, w["caps"], w["lens"])


def test_8_windows_against_the_referee(world):
    w, jobs = world, world["jobs"]
    P = w[True]
    lists = {}
    for gate in ("all", "winner"):
        for cross in (0, 300, 1000):
            want = _windows_ref(w, P, jobs, gate, cross=cross)
            got = windows(w, P, jobs, gate, cross=cross)
            _same(got[:3], want[:3])
            assert np.array_equal(got[3], want[3]) and len(want[0]) >= 5
            lists[gate, cross] = _bytes(want)
    print("windows' lists that differ from (all, 0):", [k for k in lists if lists[k] != lists["all", 0]])
    assert lists["all", 0] != lists["all", 1000]  # the cross limit acts on the job list
    want = _windows_ref(w, P, jobs, "all", cross=300, md=4)
    assert len(want[0]) == 4
    got = windows(w, P, jobs, "all", cross=300, md=4)
    _same(got[:3], want[:3])
    tr = np.array(jobs, dtype=np.int32)  # translations only: a0 = 0, na = 1
    tr[:, 1], tr[:, 2] = 0, 1
    T = w[False]
    want = _windows_ref(w, T, tr, "all", cross=600)
    got = windows(w, T, tr, "all", cross=600)
    _same(got[:3], want[:3])
    assert np.array_equal(got[3], want[3]) and len(want[0]) >= 5


def test_9_refined_is_its_composition(world):
    import openfdcm_amd as fd
    w = world
    coarse, fine = np.array([0.0, 0.3, -0.4]), np.deg2rad(np.arange(-30, 31, 6.0))
    kw = dict(penalty=fd.DefaultPenalty(), line_caps=w["caps"], margin=1)
    seeds = fd.exhaustive_detect_objects(w["dev"], w["tmpls"], w["obj"], INF, overlap=1.0, stride=w["probe"].STRIDE, max_detections=48,
                                         angles=coarse, **kw)
    jobs = fd.pose_windows(seeds, coarse, fine, fd.template_pivots(w["tmpls"]), 2, 2, 2)
    out = dict(return_boxes=True, return_matched=True, return_jobs=True, return_objects=True)
    want = fd.exhaustive_detect_windows_objects(w["dev"], w["tmpls"], jobs, w["obj"], w["ms"], overlap=0.3, cross_overlap=0.6, angles=fine,
                                                min_matched=w["omm"], gate="all", **out, **kw)
    got = fd.exhaustive_detect_refined_objects(w["dev"], w["tmpls"], w["obj"], w["ms"], coarse, fine, w["probe"].STRIDE, 2, 2, 2,
                                               coarse_max_detections=48, cross_overlap=0.6, min_matched=w["omm"], gate="all", **out, **kw)
    assert len(got) == 5 and len(got[0]) >= 1 and got[0].records().tobytes() == want[0].records().tobytes()
    assert _bytes(got[1:]) == _bytes(want[1:]) and np.array_equal(got[4], w["obj"][got[0].records()["tmpl_idx"]])


def test_10_arguments_that_need_the_handles(world):
    from openfdcm_amd import _capi as capi
    w = world
    P = w[True]
    for bad in (5, -1, 1 << 20):
        obj = w["obj"].copy()
        obj[7] = bad
        for call in (lambda: detect(w, P, "all", obj=obj), lambda: windows(w, P, w["jobs"], "all", obj=obj),
                     lambda: P.dev.best_map_objects(w["tset"], P.grid, obj, 5, P.cs, P.piv)):
            with pytest.raises(capi.FdcmError, match=r"objects: an entry is outside \[0, n_objects\)"):
                call()
    # five objects on 2^24 points: over the bound although the grid alone is under it
    big = (0, 0, 1 << 12, 1 << 12, 1, 1)
    with pytest.raises(capi.FdcmError, match=r"n_objects \* nx \* ny must be at most 2\^26"):
        P.dev.exhaustive_detect_objects(w["tset"], big, w["obj"], w["ms"], 5, P.cs, P.piv)
    with pytest.raises(capi.FdcmError, match=r"n_objects \* nx \* ny must be at most 2\^26"):
        P.dev.best_map_objects(w["tset"], big, w["obj"], 5, P.cs, P.piv)
    _same(detect(w, P, "all"), ref_detect(w, P, "all"))  # and a valid call afterwards


def test_11_empty_inputs(world):
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = world
    P = w[True]
    none = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for dev, tset, obj in [(none, w["tset"], w["obj"]), (w["dev"], DeviceTemplates([]), np.zeros(0, dtype=np.int32))]:
        piv = P.piv if tset is w["tset"] else None
        got = dev.exhaustive_detect_objects(tset, (0, 0, 5, 5, 1, 1), obj, INF, 5, P.cs, piv, boxes=True, min_matched=0.5, matched=True,
                                            gate="all")
        assert [len(p) for p in got] == [0, 0, 0]
        got = dev.exhaustive_detect_windows_objects(tset, w["jobs"][:9], obj, INF, 5, P.cs, piv, wrap=True, min_matched=0.5, boxes=True,
                                                    matched=True, job_index=True, gate="all")
        assert [len(p) for p in got] == [0, 0, 0, 0]
        s, p, fr = dev.best_map_objects(tset, (0, 0, 5, 4, 1, 1), obj, 5, P.cs, piv, min_matched=0.5, matched=True)
        assert np.isnan(s).all() and (p == -1).all() and np.isnan(fr).all() and fr.shape == (5, 4, 5)
    got = w["dev"].exhaustive_detect_windows_objects(w["tset"], np.zeros((0, 7), np.int32), w["obj"], INF, 5, P.cs, P.piv, boxes=True)
    assert [len(p) for p in got] == [0, 0]


def _probe(env, ms):
    out = subprocess.run([sys.executable, PROBE, "--max-score", ",".join(float(v).hex() for v in ms)], capture_output=True, text=True,
                         timeout=300, env={**{k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("objects_probe ")][-1].split()
    return line[1], int(line[3])


def test_12_flat_addresses_give_the_same_bytes(world):
    """In fresh processes (the switches are read once): the 64-bit address forms of the kernels the calls with objects run."""
    assert not any(k.startswith("FDCM_") for k in os.environ)
    w = world
    P = w[True]
    ms = [float(v) for v in w["ms"]]
    planes, dense, win = w["op"].calls(w["dev"], w["tset"], w["cs"], w["piv"], w["jobs"], ms, w["probe"])
    assert _bytes(planes) == _bytes(ref_planes(w, P, "all"))
    _same(dense, ref_detect(w, P, "all", cross=w["op"].CROSS))
    want = _windows_ref(w, P, w["jobs"], "all", cross=w["op"].CROSS)
    _same(win[:3], want[:3])
    default = (w["probe"].digest(planes + dense + win), len(dense[0]) + len(win[0]))
    assert default[1] > 20
    assert _probe({"FDCM_MATCHED_FLAT": "1"}, ms) == default
    assert _probe({"FDCM_WINDOWS_FLAT": "1"}, ms) == default


def test_13_two_threads_take_turns_and_history_does_not_matter(world):
    w = world
    P = w[True]
    calls = [lambda: detect(w, P, "all", cross=600), lambda: windows(w, P, w["jobs"], "all", cross=600),
             lambda: P.dev.best_map_objects(w["tset"], P.grid, w["obj"], 5, P.cs, P.piv, penalty=DEFAULT, min_matched=w["omm"], matched=True),
             lambda: detect(w, P, "winner", cross=0)]
    first = [_bytes(c()) for c in calls]
    P.dev.exhaustive_detect_all(w["tset"], (-20, -20, 70, 90, 1, 1), None, None, max_detections=64, boxes=True)
    assert [_bytes(c()) for c in calls] == first
    got, errors = {}, []

    def worker(k):
        try:
            for it in range(3):
                got[k, it] = [_bytes(c()) for c in (calls if k == 0 else calls[::-1])]
        except Exception as e:  # noqa: BLE001 -- reported below, on the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for (k, it), b in got.items():
        assert (b if k == 0 else b[::-1]) == first
    assert len(got) == 6
