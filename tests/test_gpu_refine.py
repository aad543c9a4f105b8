"""GPU tests of fdcm_matches_refine (include/fdcm.h, "Match lists: refinement"): the refined records and their poses equal the
referee (tests/refine_ref.py: numpy and Python integers on the volume, nothing from the kernels) byte for byte -- there is no
tolerance to choose; a NaN compares as the one quiet NaN.  The two maps of test_gpu_matches.World (a line-built one of about
117 pixels, an adopted 70 x 37 volume that holds a NaN and an infinity), templates of 0 to 130 lines, the four kinds of caps,
lists of 1, 3, 4, 5, 255, 256 and 257 records (the four waves of a workgroup, and a workgroup boundary) and the windows of
refine_cases.WINDOWS, the last of 5 x 19 points: more than one 4 x 16 patch per plane and more than 256 poses per record;
centre both -1 and in the table, pivots both NULL and "center".  Then the identities with verify_matches and
exhaustive_window_search, the input and output forms, the switches and FDCM_POISON in fresh processes
(tools/refine_probe.py), and the scene of refine_cases.py end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases as MC
import match_ref as R
import refine_cases as RC
import refine_ref as RR
import rotation_ref as ROT
from helpers import ROOT
from test_gpu_matches import MAPS, world

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "refine_probe.py")
N_REF = max(RC.LENGTHS)


def setting(wi, k):
    """(cs or None, pivots or None, centre) of window wi's k-th run: centre in the table or -1, pivots NULL or "center", in turn."""
    na = RC.WINDOWS[wi][0]
    centred, pivoted = (wi + k) % 2 == 0, ((wi + k) // 2) % 2 == 0
    if wi == 0:
        return None, None, 0 if centred else -1
    cs = RC.table(na, centred)
    return cs, pivoted, RC.centre_of(cs)


@functools.lru_cache(maxsize=None)
def referee(name, wi, k):
    w = world(name)
    na, hx, hy, sx, sy = RC.WINDOWS[wi]
    cs, pivoted, centre = setting(wi, k)
    return RR.refine(w.vol, w.keys, w.t, w.tmpls, w.recs[:N_REF], w.base, cs=cs, pivots=RC.centre_pivots(w.tmpls) if pivoted else None,
                     centre=centre, hx=hx, hy=hy, sx=sx, sy=sy, caps=w.caps(MC.CAPS[k]))


def device(w, wi, k, recs, **kw):
    na, hx, hy, sx, sy = RC.WINDOWS[wi]
    cs, pivoted, centre = setting(wi, k)
    return w.dev.refine_matches(w.tset(MC.CAPS[k]), recs, cs=cs, pivots=RC.centre_pivots(w.tmpls) if pivoted else None, centre=centre, hx=hx,
                                hy=hy, sx=sx, sy=sy, tmpl_index_base=w.base, poses=True, **kw)


@pytest.mark.parametrize("wi", range(len(RC.WINDOWS)))
@pytest.mark.parametrize("name", MAPS)
def test_refine_equals_the_referee(name, wi):
    w = world(name)
    seen = set()
    for k in range(len(MC.CAPS)):
        want, wp, partial = referee(name, wi, k)
        cs, pivoted, centre = setting(wi, k)
        seen.add((centre >= 0, bool(pivoted)))
        if RC.WINDOWS[wi] == RC.CHECK_WINDOW and MC.CAPS[k] == "none" and centre >= 0:
            RC.check_conditions(want, wp, partial, centre)      # on this map's own volume, as test_refine_definition.py on the oracle's
        for n in RC.LENGTHS:
            got, gp = device(w, wi, k, w.recs[:n])
            assert MC.same_records(got, want[:n]) and gp.dtype == np.int32 and np.array_equal(gp, wp[:n]), \
                (n, MC.CAPS[k], np.flatnonzero(np.any(gp != wp[:n], axis=1))[:5], np.flatnonzero(MC.canon(got["score"]) != MC.canon(want["score"][:n]))[:5])
    assert {c for c, _ in seen} == {True, False} and (wi == 0 or {p for _, p in seen} == {True, False})
    if name == "adopted" and wi == 0:
        s = referee(name, 0, 0)[0]["score"]
        assert np.isinf(s).any()          # the volume's infinity is reached; a NaN score has no key


@pytest.mark.parametrize("kind", MC.CAPS)
@pytest.mark.parametrize("name", MAPS)
def test_no_table_and_no_window_is_verify_matches(name, kind):
    w = world(name)
    s = w.dev.verify_matches(w.tset(kind), w.recs, tmpl_index_base=w.base)[0]
    t = w.recs["tmpl_idx"].astype(np.int64) - w.base
    lines = np.array([0 <= ti < len(w.tmpls) and w.tmpls[ti].shape[1] > 0 for ti in t])
    want = np.where(lines, s, np.float32(np.nan)).astype(np.float32)      # (a template without lines has s = +0 and no winner)
    for centre in (0, -1):
        got, pose = w.dev.refine_matches(w.tset(kind), w.recs, centre=centre, tmpl_index_base=w.base, poses=True)
        assert len(got) == 700 and MC.same_floats(got["score"], want) and np.array_equal(got["tmpl_idx"], w.recs["tmpl_idx"])
        assert MC.same_floats(got["transform"], w.recs["transform"])
        won = ~np.isnan(want)
        assert won.sum() > 300 and np.all(pose[won] == (0, 0, 0)) and np.all(pose[~won] == (-1, 0, 0))


@pytest.mark.parametrize("name", MAPS)
def test_identity_with_the_pose_windows(name):
    """Records {1, 0, 0, 0, 1, 0}: the k = 1 records of exhaustive_window_search for the job (t, 0, na, -hx sx, -hy sy, 2 hx + 1,
    2 hy + 1).  This holds the device-posed lines against the host-posed ones."""
    from openfdcm_amd.engine import DeviceTemplates
    w = world(name)
    rng = np.random.default_rng(12)
    tm = [(t + np.float32([[20.0], [8.0], [20.0], [8.0]])).astype(np.float32) for t in MC.template_set(13)]
    cs = RC.cs_of([0.3, -0.7, 1.9, 0.02])
    pv = RC.centre_pivots(tm)
    for pivots in (None, pv):
        assert all(np.all(q != 0) for q in ROT.rotated_set(tm, cs, pivots))
    n = 60
    ti = rng.integers(0, len(tm), size=n)
    recs = R.records(ti, np.zeros(n), [[1, 0, 0, 0, 1, 0]] * n)
    won = 0
    for caps in (None, MC.caps_of(tm, "mixed")):
        tset = DeviceTemplates(tm, line_caps=caps)
        for (na, hx, hy, sx, sy), pivots in (((4, 2, 9, 1, 1), pv), ((3, 1, 1, 2, 3), None), ((1, 0, 0, 1, 1), pv)):
            got, pose = w.dev.refine_matches(tset, recs, cs=cs[:na], pivots=pivots, centre=-1, hx=hx, hy=hy, sx=sx, sy=sy, poses=True)
            jobs = np.stack([ti, np.zeros(n), np.full(n, na), np.full(n, -hx * sx), np.full(n, -hy * sy), np.full(n, 2 * hx + 1),
                             np.full(n, 2 * hy + 1)], axis=1).astype(np.int32)
            win, offs = w.dev.exhaustive_window_search(tset, jobs, cs=cs[:na], pivots=pivots, sx=sx, sy=sy, k=1)
            for q in range(n):
                if offs[q + 1] == offs[q]:
                    assert np.isnan(got["score"][q]) and tuple(pose[q]) == (-1, 0, 0)
                    continue
                r = win[offs[q]]
                assert r["score"].tobytes() == got["score"][q].tobytes() and np.array_equal(r["transform"], got["transform"][q])
                e, i, j = pose[q]
                M = ROT.rot_matrix(cs[e, 0], cs[e, 1], *((0.0, 0.0) if pivots is None else pivots[ti[q]]))
                assert np.array_equal(r["transform"], np.float32([M[0, 0], M[0, 1], M[0, 2] + np.float32(i * sx), M[1, 0], M[1, 1],
                                                                   M[1, 2] + np.float32(j * sy)]))
                won += 1
    assert won > 100


def test_the_input_and_output_forms():
    import torch
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import search_into, search_raw
    w = world("lines")
    raw = search_raw(w.dev, w.tset(), w.scene, 4, 4, 1, 10, 7)
    assert len(raw) > 100
    cs, pv = RC.table(3, True), RC.centre_pivots(w.tmpls)
    kw = dict(cs=cs, pivots=pv, hx=2, hy=1, tmpl_index_base=7, poses=True)
    want, wp, _ = RR.refine(w.vol, w.keys, w.t, w.tmpls, raw, 7, cs=cs, pivots=pv, centre=1, hx=2, hy=1)
    assert (wp[:, 0] >= 0).sum() > 50 and np.any(wp[:, 1:] != 0, axis=1).sum() > 20
    for form in (dict(matches=None), dict(matches=raw)):       # the last search, host records
        got, gp = w.dev.refine_matches(w.tset(), **form, **kw)
        assert MC.same_records(got, want) and np.array_equal(gp, wp), form.keys()
    buf = torch.empty(w.tset().capacity(w.scene.shape[1], 4, 4) * 32, dtype=torch.uint8, device="cuda")
    n = search_into(w.dev, w.tset(), w.scene, 4, 4, _capi.BATCH_OPTIMIZE, 10, 7, buf.data_ptr())
    assert n == len(raw)
    got, gp = w.dev.refine_matches(w.tset(), device_ptr=buf.data_ptr(), n=n, **kw)       # device records, host output
    assert MC.same_records(got, want) and np.array_equal(gp, wp)
    assert np.array_equal(np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=R.MATCH_DTYPE), raw)   # read in place, not written
    other = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    none, gp = w.dev.refine_matches(w.tset(), raw, out_device_ptr=other.data_ptr(), **kw)               # host records, device output
    assert none is None and np.array_equal(gp, wp)
    assert MC.same_records(np.frombuffer(other.cpu().numpy().tobytes(), dtype=R.MATCH_DTYPE), want)
    none, gp = w.dev.refine_matches(w.tset(), device_ptr=buf.data_ptr(), n=n, out_device_ptr=buf.data_ptr(), **kw)   # in place
    assert none is None and np.array_equal(gp, wp)
    refined = np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=R.MATCH_DTYPE)
    assert MC.same_records(refined, want)
    # the refined device buffer goes straight on to detect_matches
    dk = dict(overlap_permille=300, penalty=0, tmpl_index_base=7, indices=True, boxes=True, matched=True)
    a = w.dev.detect_matches(w.tset(), device_ptr=buf.data_ptr(), n=n, **dk)
    b = w.dev.detect_matches(w.tset(), want, **dk)
    assert len(b[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_runs_the_public_call_and_empty_inputs():
    import openfdcm_amd as fd
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = world("adopted")
    recs = np.array(w.recs)
    recs["tmpl_idx"] -= w.base
    angles = fd.delta_angles(1, np.deg2rad(1.5))
    caps = w.caps("scalar")
    first = fd.refine_matches(w.dev, w.tmpls, fd.MatchList(recs), angles=angles, half_x=1, half_y=2, stride=(2, 1), line_caps=caps, return_poses=True)
    assert isinstance(first[0], fd.MatchList) and first[1].shape == (700, 3)
    want = RR.refine(w.vol, w.keys, w.t, w.tmpls, recs[:257], 0, cs=RC.cs_of(angles), pivots=RC.centre_pivots(w.tmpls), centre=1, hx=1, hy=2,
                     sx=2, sy=1, caps=caps)
    assert MC.same_records(first[0].records()[:257], want[0]) and np.array_equal(first[1][:257], want[1])
    for _ in range(2):
        again = fd.refine_matches(w.dev, w.tmpls, recs, angles=angles, half_x=1, half_y=2, stride=(2, 1), line_caps=caps, return_poses=True)
        assert again[0].records().tobytes() == first[0].records().tobytes() and np.array_equal(again[1], first[1])
    only = fd.refine_matches(w.dev, w.tmpls, recs, angles=angles, half_x=1, half_y=2, stride=(2, 1), line_caps=caps)
    assert isinstance(only, fd.MatchList) and only.records().tobytes() == first[0].records().tobytes()
    # nothing is written for an empty list, an empty set or an empty map: no record has a winner
    none = np.zeros(0, dtype=R.MATCH_DTYPE)
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts, rr in [(w.dev, w.tset(), none), (w.dev, DeviceTemplates([]), w.recs[:5]), (empty_map, w.tset(), w.recs[:5])]:
        out, pose = fm.refine_matches(ts, rr, hx=1, hy=1, poses=True)
        assert len(out) == len(rr) and np.isnan(out["score"]).all() and np.all(pose == (-1, 0, 0)) and MC.same_floats(out["transform"], rr["transform"])
    bad = RC.centre_pivots(w.tmpls)
    bad[3, 1] = np.inf
    with pytest.raises(_capi.FdcmError, match="pivots must be finite"):
        w.dev.refine_matches(w.tset(), w.recs, cs=RC.table(3, True), pivots=bad)
    with pytest.raises(_capi.FdcmError, match="at most 65536"):
        w.dev.refine_matches(w.tset(), w.recs, cs=RC.table(3, True), hx=100, hy=100)


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=240, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("refine_probe ")][-1].split()


def test_switches_and_poison_in_fresh_processes():
    """tools/refine_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after a
    failure (an assertion ends the test).  The digests equal this process's own, and its two runs agree."""
    spec = __import__("importlib.util").util.spec_from_file_location("refine_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, winners, moved = probe.run()
    assert winners > 2000 and moved > 500
    assert probe.run() == (digest, winners, moved)
    for env in ({"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_MATCHED_FLAT": "1"}, {"FDCM_FORCE_HOST_BINS": "1"}, {"FDCM_REFINE_PART": "100"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == winners and int(line[5]) == moved, (env, line)


def test_the_scene_end_to_end():
    """The scene of refine_cases.py: every perturbed record comes back at the planted pose with the unperturbed record's score,
    and detect_matches on the refined list returns one record whose transform is the true one as floats."""
    import openfdcm_amd as fd
    lines, tmpls, true, recs, planted = RC.scene()
    fm = fd.build_cpu_featuremap(lines, fd.Dt3CpuParameters(depth=RC.BUILD["depth"], dt3Coeff=RC.BUILD["coeff"], padding=RC.BUILD["padding"]))
    dev = fm._fm
    angles = fd.delta_angles(RC.HALF_STEPS, RC.STEP)
    got, pose = fd.refine_matches(fm, tmpls, recs, angles=angles, pivot=RC.PIVOT, half_x=RC.HALF_X, half_y=RC.HALF_Y, return_poses=True)
    want, wp, _ = RR.refine(dev.volume(), dev.keys, dev.scene_translation, tmpls, recs, cs=RC.cs_of(angles), pivots=RC.PIVOT,
                            centre=RC.HALF_STEPS, hx=RC.HALF_X, hy=RC.HALF_Y)
    assert MC.same_records(got.records(), want) and np.array_equal(pose, wp)
    assert np.array_equal(pose, planted)
    s_true = fd.verify_matches(fm, tmpls, true)[0]
    assert np.all(got.records()["score"] == s_true[0])
    # "center" is the same pivot: the part's bounding box
    assert fd.refine_matches(fm, tmpls, recs, angles=angles, half_x=RC.HALF_X, half_y=RC.HALF_Y).records().tobytes() == got.records().tobytes()
    one = fd.detect_matches(fm, tmpls, got, overlap=0.3)
    assert len(one) == 1
    kept = one.records()[0]
    unmoved = int(np.flatnonzero(np.all(planted == (RC.HALF_STEPS, 0, 0), axis=1))[0])
    assert np.array_equal(kept["transform"], true["transform"][0]) and kept["transform"].tobytes() == got.records()["transform"][unmoved].tobytes()
