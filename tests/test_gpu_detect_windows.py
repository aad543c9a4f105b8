"""GPU tests of the detections over pose windows (include/fdcm.h, "Detections over pose windows").  The referee is the
numpy statement window_detect_ref.py on planes other tests hold to their definitions: the score maps of the set (with its
caps) and the uncapped cost maps of its lines on a stride-1 master grid.  The main case (tools/window_detect_probe.py) is a
96 x 80 map with planted template instances, six templates of 0 to 8 lines, twelve angles with wrap and about 200 jobs."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import nms_ref
from capped_ref import line_cost_maps
from window_detect_ref import detect_windows_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "window_detect_probe.py")
DEFAULT, EXPONENTIAL = 0, 1
MM = 0.3       # the gate of the main case
MARGIN = 1
f32 = np.float32


def _load():
    spec = importlib.util.spec_from_file_location("window_detect_probe", PROBE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _den(lengths, penalty, tau=1.0):
    """best_denominators' rule: 1 without a penalty, max(len, 1e-6f), or std::pow of that and tau in float32 (libm's powf)."""
    lengths = np.asarray(lengths, dtype=np.float32)
    if penalty is None:
        return np.ones(len(lengths), dtype=np.float32)
    l = np.maximum(lengths, f32(1e-6))
    if penalty == DEFAULT:
        return l
    powf = C.CDLL("libm.so.6").powf
    powf.restype, powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return np.array([powf(float(v), float(tau)) for v in l], dtype=np.float32)


@pytest.fixture(scope="module")
def world():
    """The main case, its device map and, computed once and left unchanged, the planes the referee reads: per template the
    score volumes over the twelve angles and over the lines as they are, with the scalar caps and without, and the cost maps
    of every line."""
    from openfdcm_amd.engine import DeviceTemplates, line_lengths
    probe = _load()
    scene, tmpls, cs, piv, jobs = probe.case()
    dev = probe.build(scene)
    assert (dev.width, dev.height) == (96, 80) and dev.depth == 12
    X0, Y0, NX, NY = probe.MASTER
    grid = (X0, Y0, NX, NY, 1, 1)
    capped, plain = DeviceTemplates(tmpls, line_caps=probe.TAU), DeviceTemplates(tmpls)
    lens = line_lengths(tmpls)
    w = dict(probe=probe, dev=dev, tmpls=tmpls, cs=cs, piv=piv, jobs=jobs, master=probe.MASTER, lens=lens, n=len(cs),
             lengths=capped.lengths(), sets={True: capped, False: plain},
             caps={True: [f32(probe.TAU) * l for l in lens], False: [np.full(len(l), np.inf, dtype=np.float32) for l in lens]})
    has = [tm.shape[1] > 0 for tm in tmpls]
    for rot in (True, False):
        cost, off = line_cost_maps(dev, tmpls, grid, cs if rot else None, piv if rot else None)
        cost = cost if rot else cost[:, None]
        w["costs", rot] = [cost[off[t]:off[t + 1]] if has[t] else None for t in range(len(tmpls))]
        for cap in (True, False):
            v = dev.rotation_score_map(w["sets"][cap], grid, cs, piv) if rot else dev.score_map(w["sets"][cap], grid)[:, None]
            v.setflags(write=False)
            w["vols", rot, cap] = [v[t] if has[t] else None for t in range(len(tmpls))]
    assert sum(int((~np.isnan(v)).sum()) for v in w["vols", True, True] if v is not None) > 100000
    return w


def _tr_jobs(jobs):
    """The jobs as translation-only jobs: a0 = 0, na = 1."""
    j = np.array(jobs, dtype=np.int32)
    j[:, 1], j[:, 2] = 0, 1
    return j


def _want(w, jobs, rot=True, cap=True, penalty=DEFAULT, tau=1.0, max_score=np.inf, max_det=4096, permille=300, mm=0.0, stride=(1, 1),
          margin=MARGIN, base=0):
    cs, piv = (w["cs"], w["piv"]) if rot else (None, None)
    boxes = nms_ref.footprints(w["tmpls"], cs, piv, margin=margin)
    return detect_windows_ref(w["vols", rot, cap], w["master"], jobs, cs, piv, stride[0], stride[1], _den(w["lengths"], penalty, tau), boxes,
                              max_score, max_det, permille, mm, w["costs", rot], w["caps"][cap], w["lens"], base=base)


def _got(w, jobs, rot=True, cap=True, penalty=DEFAULT, tau=1.0, max_score=np.inf, max_det=4096, permille=300, mm=0.0, stride=(1, 1),
         margin=MARGIN, base=0, dev=None):
    cs, piv = (w["cs"], w["piv"]) if rot else (None, None)
    return (dev or w["dev"]).exhaustive_detect_windows(
        w["sets"][cap], jobs, cs, piv, sx=stride[0], sy=stride[1], wrap=True, max_score=max_score, max_detections=max_det,
        overlap_permille=permille, margin=margin, penalty=penalty, tau=tau, min_matched=mm if mm else None, tmpl_index_base=base,
        boxes=True, matched=True, job_index=True)


def _same(got, want):
    rec, box, frac, ji = got
    wrec, wbox, wfrac, wji = want[:4]
    assert np.array_equal(ji, wji)
    assert np.array_equal(rec["tmpl_idx"], wrec["tmpl_idx"])
    assert rec["score"].tobytes() == wrec["score"].tobytes()
    assert rec["transform"].tobytes() == wrec["transform"].tobytes()
    assert np.array_equal(box, wbox) and box.dtype == np.int32
    assert frac.tobytes() == wfrac.tobytes()


def _bytes(got):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in got)


def test_the_main_case_against_the_numpy_statement(world):
    w, jobs = world, world["jobs"]
    assert 190 <= len(jobs) <= 220
    pts = jobs[:, 2] * jobs[:, 5] * jobs[:, 6]
    assert pts.max() == 65536 and (pts == 1).sum() >= 40 and ((jobs[:, 1] + jobs[:, 2]) > w["n"]).sum() >= 2
    assert len({tuple(j) for j in jobs}) < len(jobs)  # duplicates
    every = _want(w, jobs, permille=1000)
    q = np.sort(every[0]["score"])
    thr = float(q[int(len(q) * 0.7)])
    print("winners", len(q), "threshold", thr)
    for permille in (0, 300, 1000):
        for mm in (0.0, MM):
            for max_score in (np.inf, thr):
                want = _want(w, jobs, max_score=max_score, permille=permille, mm=mm)
                print("overlap", permille, "min_matched", mm, "max_score", max_score, want[4])
                _same(_got(w, jobs, max_score=max_score, permille=permille, mm=mm), want)
                if (permille, mm, max_score) == (300, MM, thr):  # not vacuous: the statement alone says so
                    c = want[4]
                    assert c["detections"] >= 20 and c["threshold"] >= 1 and c["gate"] >= 1 and c["suppressed"] >= 1 and c["no_winner"] >= 1
                    assert 0 < np.isfinite(want[2]).sum() and (want[2] < 1).any() and (want[2] >= f32(MM)).all()


def test_other_tables_caps_penalties_strides_and_list_bounds(world):
    w, jobs = world, world["jobs"]
    tr = _tr_jobs(jobs)
    n_tr = 0
    for cap in (True, False):
        want = _want(w, tr, rot=False, cap=cap, mm=MM)
        _same(_got(w, tr, rot=False, cap=cap, mm=MM), want)          # angles=None
        n_tr += len(want[0])
        assert np.all(want[0]["transform"][:, [0, 1, 3, 4]] == [1, 0, 0, 1])
    assert n_tr > 20
    want = _want(w, jobs, cap=False, mm=0.5, max_score=40.0)
    _same(_got(w, jobs, cap=False, mm=0.5, max_score=40.0), want)    # line_caps=None: every line is matched, frac = 1
    assert len(want[0]) > 10 and np.all(want[2] == 1)
    for penalty, tau in [(None, 1.0), (DEFAULT, 1.0), (EXPONENTIAL, 1.5)]:
        want = _want(w, jobs, penalty=penalty, tau=tau, mm=MM, base=7)
        _same(_got(w, jobs, penalty=penalty, tau=tau, mm=MM, base=7), want)
        assert len(want[0]) > 10
    small = jobs[jobs[:, 5] * jobs[:, 6] <= 64]                      # windows that stay inside the master grid at strides (2, 3)
    want = _want(w, small, stride=(2, 3), mm=MM, margin=0)
    _same(_got(w, small, stride=(2, 3), mm=MM, margin=0), want)
    assert len(want[0]) > 10
    cands = len(_want(w, jobs, permille=1000, mm=MM)[0])
    for max_det in (1, cands, cands - 1):
        for permille in (300, 1000):
            want = _want(w, jobs, permille=permille, mm=MM, max_det=max_det)
            _same(_got(w, jobs, permille=permille, mm=MM, max_det=max_det), want)
            assert len(want[0]) == (max_det if permille == 1000 else min(max_det, len(want[0])))


def test_identity_1_the_window_search_penalised_and_ordered(world):
    from openfdcm_amd import _capi
    w, jobs = world, world["jobs"]
    dev, tset = w["dev"], w["sets"][True]
    for penalty, tau in [(DEFAULT, 1.0), (EXPONENTIAL, 1.5), (None, 1.0)]:
        rec, off = dev.exhaustive_window_search(tset, jobs, w["cs"], w["piv"], wrap=True, k=1, tmpl_index_base=0)
        rec = np.array(rec)
        job_of = np.repeat(np.arange(len(jobs)), np.diff(off))
        if penalty is not None:
            lens = np.ascontiguousarray(w["lengths"], dtype=np.float32)
            _capi.check(_capi.lib().fdcm_penalize(int(penalty), float(tau), C.c_void_p(rec.ctypes.data), len(rec), _capi.fptr(lens), len(lens)))
        order = np.argsort(rec["score"].view(np.uint32), kind="stable")  # (score bits, job): the records are in job order
        got = dev.exhaustive_detect_windows(tset, jobs, w["cs"], w["piv"], wrap=True, max_detections=len(rec) + 3, overlap_permille=1000,
                                            penalty=penalty, tau=tau, job_index=True)
        assert len(rec) > 100 and got[0].tobytes() == rec[order].tobytes() and np.array_equal(got[1], job_of[order])


def test_identity_2_one_point_jobs_are_the_dense_detector(world):
    w = world
    dev, tset, cs, piv = w["dev"], w["sets"][True], w["cs"], w["piv"]
    grid = (8, 6, 46, 38, 1, 1)
    n = 0
    for rot in (True, False):
        c, pv = (cs, piv) if rot else (None, None)
        A = len(cs) if rot else 1
        scores, pairs = dev.best_map(tset, grid, c, pv, penalty=DEFAULT)
        g = np.nonzero(pairs.reshape(-1) >= 0)[0]
        u = pairs.reshape(-1)[g]
        jobs = np.stack([u // A, u % A, np.ones_like(u), grid[0] + g % grid[2], grid[1] + g // grid[2], np.ones_like(u), np.ones_like(u)],
                        axis=1).astype(np.int32)
        assert len(jobs) > 1000
        thr = float(np.sort(scores.reshape(-1)[g])[len(g) // 3])
        for max_score, mm, permille, max_det in [(np.inf, None, 300, 4096), (thr, 0.3, 300, 4096), (thr, 0.5, 0, 4096), (np.inf, 0.2, 1000, 50)]:
            want = dev.exhaustive_detect_all(tset, grid, c, pv, max_score=max_score, max_detections=max_det, overlap_permille=permille,
                                             margin=2, penalty=DEFAULT, min_matched=mm, boxes=True, matched=True)
            got = dev.exhaustive_detect_windows(tset, jobs, c, pv, max_score=max_score, max_detections=max_det, overlap_permille=permille,
                                                margin=2, penalty=DEFAULT, min_matched=mm, boxes=True, matched=True)
            assert len(want[0]) >= 2 and _bytes(got) == _bytes(want)  # (boxes of 20 pixels on a grid of 46 x 38: few survive)
            n += len(want[0])
    assert n > 100


def test_identities_3_and_4_threshold_prefix_and_disjoint_boxes(world):
    w, jobs = world, world["jobs"]
    full = _got(w, jobs, mm=MM, permille=300)
    s = full[0]["score"]
    assert len(s) >= 20 and np.all(np.diff(s.view(np.uint32).astype(np.int64)) >= 0)
    for thr in [float(s[0]), float(s[len(s) // 3]), float(np.nextafter(s[len(s) // 2], f32(0))), float(s[-1]), 0.0]:
        got = _got(w, jobs, mm=MM, permille=300, max_score=thr)
        k = int((s <= f32(thr)).sum())
        assert len(got[0]) == k and _bytes(got) == _bytes(tuple(p[:k] for p in full))
    rec, box, frac, ji = _got(w, jobs, permille=0)
    assert len(rec) >= 10
    for a in range(len(box)):
        for b in range(a + 1, len(box)):
            A, B = box[a].astype(np.int64), box[b].astype(np.int64)
            assert min(A[2], B[2]) < max(A[0], B[0]) or min(A[3], B[3]) < max(A[1], B[1]), (a, b)


def test_the_same_bytes_whatever_ran_before_and_on_a_fresh_handle(world):
    w, jobs = world, world["jobs"]
    kw = dict(mm=MM, permille=300, max_score=2.6)
    first = _bytes(_got(w, jobs, **kw))
    assert first == _bytes(_got(w, jobs, **kw))
    w["dev"].exhaustive_detect_all(w["sets"][False], (-20, -20, 120, 100, 1, 1), w["cs"], w["piv"], max_detections=64, boxes=True)
    w["dev"].exhaustive_window_search(w["sets"][True], jobs[:50], w["cs"], w["piv"], wrap=True, k=64)
    assert first == _bytes(_got(w, jobs, **kw))
    fresh = w["probe"].build(w["probe"].case()[0])
    assert first == _bytes(_got(w, jobs, dev=fresh, **kw))


def test_a_list_in_two_calls_merges_to_the_list_in_one(world):
    """The candidates of each half with their keys' scores, boxes and jobs (overlap 1: nothing suppressed), merged by the
    numpy rule in Python integers, are the detections of the whole list."""
    w, jobs = world, world["jobs"]
    half = len(jobs) // 2
    cand = []
    for j0, part in [(0, jobs[:half]), (half, jobs[half:])]:
        rec, box, frac, ji = _got(w, part, mm=MM, permille=1000)
        cand += [((int(rec["score"][l:l + 1].view(np.uint32)[0]) << 32) | (j0 + int(ji[l])), [int(v) for v in box[l]], rec[l], frac[l])
                 for l in range(len(rec))]
    left = sorted(cand, key=lambda c: c[0])
    out = []
    while left:
        d = left.pop(0)
        out.append(d)
        keep = []
        for c in left:
            G, F = c[1], d[1]
            inter = max(0, min(G[2], F[2]) - max(G[0], F[0]) + 1) * max(0, min(G[3], F[3]) - max(G[1], F[1]) + 1)
            union = (G[2] - G[0] + 1) * (G[3] - G[1] + 1) + (F[2] - F[0] + 1) * (F[3] - F[1] + 1) - inter
            if not 1000 * inter > 300 * union:
                keep.append(c)
        left = keep
    rec, box, frac, ji = _got(w, jobs, mm=MM, permille=300)
    assert len(out) == len(rec) >= 20
    assert [c[0] & 0xffffffff for c in out] == ji.tolist() and [c[1] for c in out] == box.tolist()
    assert b"".join(c[2].tobytes() for c in out) == rec.tobytes() and b"".join(c[3].tobytes() for c in out) == frac.tobytes()


def _probe(env):
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=300,
                         env={**{k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("window_detect_probe ")][-1].split()
    return line[1], int(line[3])


def test_flat_addresses_and_many_parts_give_the_same_bytes(world):
    """In fresh processes (the switches are read once): the 64-bit address form of the scoring, the winners' pass and the
    fractions, and the job list scored in parts of 5 planes and 20 KB of tables, dozens of them."""
    assert not any(k.startswith("FDCM_") for k in os.environ)
    default = world["probe"].run()
    assert default[1] > 200
    assert _probe({"FDCM_MATCHED_FLAT": "1"}) == default
    assert _probe({"FDCM_WINDOWS_BATCH": "5"}) == default


def test_refined_is_its_composition_and_pose_windows_takes_detect_records(world):
    import openfdcm_amd as openfdcm
    probe = world["probe"]
    scene, tmpls = probe.case()[:2]
    fm = openfdcm.build_cpu_featuremap(scene, openfdcm.Dt3CpuParameters(depth=12, dt3Coeff=5.0, padding=1.0))
    coarse, fine = probe.angles(), np.deg2rad(np.arange(72) * 5.0)
    pen = openfdcm.DefaultPenalty()
    kw = dict(penalty=pen, line_caps=probe.TAU, margin=1)
    seeds = openfdcm.exhaustive_detect_all(fm, tmpls, float("inf"), overlap=1.0, stride=2, max_detections=64, angles=coarse, **kw)
    assert len(seeds) == 64
    piv = openfdcm.template_pivots(tmpls)
    jobs = openfdcm.pose_windows(seeds, coarse, fine, piv, 3, 2, 2, wrap=True)
    assert jobs.shape == (64, 7) and jobs.dtype == np.int32 and np.all(jobs[:, 2] == 7) and np.all(jobs[:, 5:] == 5)
    assert np.array_equal(jobs[:, 0], seeds.records()["tmpl_idx"])
    # a detect record is read as the rotation search's: the one-point job at its pose finds the record's own transform
    at = openfdcm.pose_windows(seeds, coarse, coarse, piv, 0, 0, 0)
    back, off = openfdcm.exhaustive_window_search(fm, tmpls, at, angles=coarse, line_caps=probe.TAU)
    assert off.tolist() == list(range(65)) and back.records()["transform"].tobytes() == seeds.records()["transform"].tobytes()
    want = openfdcm.exhaustive_detect_windows(fm, tmpls, jobs, 2.5, overlap=0.3, angles=fine, wrap=True, min_matched=0.3, return_boxes=True,
                                              return_matched=True, return_jobs=True, **kw)
    got = openfdcm.exhaustive_detect_refined(fm, tmpls, 2.5, coarse, fine, 2, 3, 2, 2, coarse_max_detections=64, wrap=True, min_matched=0.3,
                                             return_boxes=True, return_matched=True, return_jobs=True, **kw)
    print("refined detections", len(got[0]), "from jobs", got[3].tolist())
    assert isinstance(got[0], openfdcm.MatchList) and 1 <= len(got[0]) < 64
    assert got[0].records().tobytes() == want[0].records().tobytes()
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got[1:], want[1:])) and len(got) == 4
    alone = openfdcm.exhaustive_detect_refined(fm, tmpls, 2.5, coarse, fine, 2, 3, 2, 2, coarse_max_detections=64, wrap=True, **kw)
    assert isinstance(alone, openfdcm.MatchList) and len(alone) >= 1


def test_bad_arguments_on_a_device_then_a_valid_call_and_empty_inputs(world):
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = world
    dev, tset, cs, piv = w["dev"], w["sets"][True], w["cs"], w["piv"]
    good = w["jobs"][:40]
    want = _bytes(_got(w, good, mm=MM))
    for bad in [[(len(w["tmpls"]), 0, 1, 0, 0, 3, 3)], [(0, 0, 13, 0, 0, 3, 3)], [(0, 12, 1, 0, 0, 3, 3)]]:
        with pytest.raises(Exception):
            dev.exhaustive_detect_windows(tset, np.int32(bad), cs, piv, wrap=True)
        assert _bytes(_got(w, good, mm=MM)) == want
    with pytest.raises(Exception):
        dev.exhaustive_detect_windows(tset, good, cs, piv, wrap=False)  # a run crosses the end of the table
    for empty in [dev.exhaustive_detect_windows(tset, np.zeros((0, 7), np.int32), cs, piv, boxes=True, matched=True, job_index=True),
                  DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
                  .exhaustive_detect_windows(tset, good, cs, piv, wrap=True, boxes=True, matched=True, job_index=True),
                  dev.exhaustive_detect_windows(DeviceTemplates([]), good, cs, None, wrap=True, boxes=True, matched=True, job_index=True)]:
        assert [len(p) for p in empty] == [0, 0, 0, 0] and empty[1].shape == (0, 4)
