"""GPU tests of scene coverage and selection of match records (include/fdcm.h, "Match lists: scene coverage and selection"): the
counts, the residual and the selection of fdcm_matches_coverage and fdcm_matches_select equal the referee's
(tests/match_coverage_ref.py: numpy and plain integers, nothing from the kernel) byte for byte -- there is no tolerance to
choose -- on the record lists of match_coverage_cases.py.  Then the 270 one-line records that cross two batches of rounds, the
section's identities on device output, the three record forms on what a real search returns, labels as array and as tensor,
empty inputs and refusals, the switches in fresh processes (tools/match_coverage_probe.py) and coverage in parts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_coverage_cases as CS
import match_coverage_ref as MC
import match_ref as MR
import select_cases as SC
import test_gpu_coverage as G
from helpers import ROOT

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "match_coverage_probe.py")


def same(got, want):
    return all(np.asarray(g).dtype == v.dtype and np.asarray(g).shape == v.shape and np.asarray(g).tobytes() == v.tobytes()
               for g, v in zip(got, want))


def cover(w, case, recs=None, labels=None, **kw):
    return w.dev.match_coverage(case.labels if labels is None else labels, w.tset, case.recs if recs is None else recs,
                                tmpl_index_base=case.base, **kw)


def select(w, case, recs=None, labels=None, **kw):
    return w.dev.select_matches(case.labels if labels is None else labels, w.tset, case.recs if recs is None else recs,
                                tmpl_index_base=case.base, residual=True, **kw)


@pytest.mark.parametrize("radius", SC.RADII)
@pytest.mark.parametrize("name", CS.WORLDS)
def test_counts_and_residual_equal_the_referee(name, radius):
    w, case = G.world(name, False), CS.case(name)
    assert np.array_equal(case.labels, w.labels) and len(case.tmpls) == len(w.tmpls)
    for tol in (0, case.m // 2):
        want_c, want_r, _ = case.coverage(radius=radius, bin_tolerance=tol)
        got_c, got_r = cover(w, case, radius=radius, bin_tolerance=tol, residual=True)
        bad = np.flatnonzero((got_c != want_c).any(axis=1)) if got_c.shape == want_c.shape else None
        assert same((got_c,), (want_c,)), (tol, bad, got_c[bad][:5], want_c[bad][:5])
        assert same((got_r,), (want_r,)), (tol, np.argwhere(got_r != want_r)[:5])
        assert same((cover(w, case, radius=radius, bin_tolerance=tol),), (want_c,))                # without the residual
    adm = want_c[:, 0] >= 0
    assert 50 <= len(want_c) <= 70 and adm.sum() >= 30 and (~adm).sum() >= 10 and np.any(want_c[adm, 1] > 0)


@pytest.mark.parametrize("name", CS.WORLDS)
def test_selection_equals_the_referee(name):
    w, case = G.world(name, False), CS.case(name)
    accepted = 0
    for cov, share, pix in SC.PARAMS:
        kw = dict(radius=2, bin_tolerance=1, min_coverage=cov, min_new=share, min_pixels=pix)
        for ms in SC.MAX_SELECTED:
            want = case.select(max_selected=ms, **kw)
            got = select(w, case, max_selected=ms, **kw)
            assert same(got, want), (cov, share, pix, ms, got[0], want[0], got[1][:4], want[1][:4])
        accepted += len(want[0])
    no_res = w.dev.select_matches(case.labels, w.tset, case.recs, tmpl_index_base=case.base, max_selected=ms, **kw)
    assert len(no_res) == 2 and same(no_res, want[:2])
    assert accepted > 24


def test_a_long_list_crosses_batches_of_rounds():
    from openfdcm_amd.engine import DeviceTemplates
    w, case = G.world("96x80-b0-d30", False), CS.long_case()
    tset = DeviceTemplates(case.tmpls)
    kw = dict(bin_tolerance=case.m // 2, **SC.LONG_KW)
    assert len(case.recs) == 270 and len(case.select(min_new=0.0, min_pixels=1, max_selected=4096, **kw)[0]) > 128
    for par in (dict(min_new=0.0, min_pixels=1), dict(min_new=0.5)):
        for ms in (64, 65, 4096):
            want = case.select(max_selected=ms, **par, **kw)
            got = w.dev.select_matches(case.labels, tset, case.recs, max_selected=ms, residual=True, **par, **kw)
            assert same(got, want), (par, ms, len(got[0]), len(want[0]))


@pytest.mark.parametrize("name", ["96x80-b5-d6", "70x37-b5-d30-bytes"])
def test_identity_1_integer_translations_are_the_pose_calls(name):
    w, case = G.world(name, False), CS.pose_case(name)
    for radius, tol, margin in [(2, 1, None), (0, 0, 40), (32, w.m // 2, 5)]:
        kw = dict(radius=radius, bin_tolerance=tol, margin=margin)
        want = w.dev.scene_coverage(w.labels, w.tset, w.poses, residual=True, **kw)
        assert same(cover(w, case, residual=True, **kw), want)
        for par in (dict(min_new=0.5), dict(min_coverage=0.3, min_new=0.0, min_pixels=3, max_selected=3)):
            assert same(select(w, case, **kw, **par), w.dev.scene_select(w.labels, w.tset, w.poses, residual=True, **kw, **par))


@pytest.mark.parametrize("name", ["96x80-b0-d30", "70x37-b5-d30"])
def test_identities_on_device_output(name):
    w, case = G.world(name, False), CS.case(name)
    # 2: explained <= edges; explained does not fall when radius or bin_tolerance grows; at m / 2 only "is an edge" matters
    prev = None
    for radius in (0, 1, 2, 7, 32):
        row = None
        for tol in (0, 1, case.m // 4, case.m // 2):
            c = cover(w, case, radius=radius, bin_tolerance=tol, margin=5)
            adm = c[:, 0] >= 0
            assert np.all(c[adm, 1] <= c[adm, 0]) and np.all(c[~adm] == -1)
            assert row is None or (np.array_equal(row[:, 0], c[:, 0]) and np.all(row[:, 1] <= c[:, 1]))
            row = c
        assert prev is None or np.all(prev[:, 1] <= row[:, 1])
        prev = row
    relabeled = np.where(case.labels < case.m, (case.labels.astype(np.int64) * 7 + 3) % case.m, case.labels).astype(np.uint8)
    assert np.array_equal(cover(w, case, labels=relabeled, radius=2, bin_tolerance=case.m // 2), cover(w, case, radius=2, bin_tolerance=case.m // 2))
    # the residual of a concatenation is the per-pixel "255 if either"
    a, b = case.recs[:25], case.recs[25:]
    kw = dict(radius=2, bin_tolerance=1, residual=True)
    (ca, ra), (cb, rb), (cc, rc) = cover(w, case, a, **kw), cover(w, case, b, **kw), cover(w, case, **kw)
    assert np.array_equal(np.concatenate([ca, cb]), cc) and np.array_equal(np.where((ra == 255) | (rb == 255), 255, case.labels), rc)
    blank = np.full_like(case.labels, 255)
    c, r = cover(w, case, labels=blank, **kw)
    assert np.all(c[c[:, 0] >= 0] == 0) and np.array_equal(r, blank) and np.array_equal(c[:, 0] >= 0, cc[:, 0] >= 0)
    # 3: scene selection's identities, device against device and against the referee

    def device_coverage(recs):
        return cover(w, case, recs, radius=2, bin_tolerance=1, margin=5, residual=True)
    for cov, share, pix in SC.PARAMS:
        kw = dict(radius=2, bin_tolerance=1, margin=5, min_coverage=cov, min_new=share, min_pixels=pix)
        full = select(w, case, max_selected=4096, **kw)
        CS.check_identities(case, full, max_selected=4096, coverage=device_coverage, **kw)
        CS.check_identities(case, full, max_selected=4096, **kw)
        for ms in (1, 2, 3, 5):
            part = select(w, case, max_selected=ms, **kw)
            assert np.array_equal(part[0], full[0][:ms]) and np.array_equal(part[1], full[1][:ms])
    # one coverage call per candidate on the running residual selects the same records
    kw = dict(radius=2, bin_tolerance=1)
    counts = cover(w, case, **kw)
    running, chosen = case.labels, []
    for j in range(len(case.recs)):
        if counts[j, 1] < 1:
            continue
        c, r = cover(w, case, case.recs[j:j + 1], labels=running, residual=True, **kw)
        if c[0, 1] >= 1 and 1000 * int(c[0, 1]) >= 500 * int(counts[j, 1]):
            running, chosen = r, chosen + [j]
    got = select(w, case, min_new=0.5, max_selected=4096, **kw)
    assert got[0].tolist() == chosen and np.array_equal(got[2], running) and len(chosen) > 3


def test_two_runs_are_byte_identical_and_the_pose_calls_are_untouched():
    for name in ("96x80-b0-d30", "70x37-b5-d30-bytes"):
        w, case = G.world(name, False), CS.case(name)
        before = (w.run(radius=2, bin_tolerance=1, margin=40, residual=True), w.dev.scene_select(w.labels, w.tset, w.poses, residual=True))
        first = (cover(w, case, radius=2, bin_tolerance=1, margin=40, residual=True), select(w, case, min_new=0.3, max_selected=4096))
        for _ in range(3):
            again = (cover(w, case, radius=2, bin_tolerance=1, margin=40, residual=True), select(w, case, min_new=0.3, max_selected=4096))
            assert same(again[0], first[0]) and same(again[1], first[1])
        after = (w.run(radius=2, bin_tolerance=1, margin=40, residual=True), w.dev.scene_select(w.labels, w.tset, w.poses, residual=True))
        assert same(after[0], before[0]) and same(after[1], before[1])


def test_the_three_record_forms_on_the_records_of_a_search():
    import torch
    import openfdcm_amd as fd
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceTemplates, search_into, search_raw
    img = SC.notch_frame()
    labels = fd.edge_labels(img, depth=30, threshold=60)
    dev = fd.build_image_featuremap(img, threshold=60)._fm
    tmpls = [G.part_template(), SC.outline(SC.BAR)]
    tset = DeviceTemplates(tmpls)
    scene = np.ascontiguousarray(np.concatenate([tmpls[0] + np.float32([*G.PART_AT] * 2)[:, None], tmpls[1] + np.float32([*SC.BAR_AT] * 2)[:, None]], axis=1))
    raw = search_raw(dev, tset, scene, 4, 4, 1, 10, 3)
    assert len(raw) > 50
    kw = dict(radius=2, bin_tolerance=1, tmpl_index_base=3, residual=True)
    want = MC.coverage(labels, dev.keys, (0, 0), dev.width, dev.height, tmpls, raw, 3, radius=2, bin_tolerance=1)[:2]
    assert (want[0][:, 0] >= 0).sum() > 20
    want_s = MC.select(labels, dev.keys, (0, 0), dev.width, dev.height, tmpls, raw, 3, radius=2, bin_tolerance=1, min_new=0.5)
    for form in (dict(matches=None), dict(matches=raw)):
        assert same(dev.match_coverage(labels, tset, **form, **kw), want), form.keys()
        assert same(dev.select_matches(labels, tset, **form, min_new=0.5, **kw), want_s), form.keys()
    buf = torch.empty(tset.capacity(scene.shape[1], 4, 4) * 32, dtype=torch.uint8, device="cuda")
    n = search_into(dev, tset, scene, 4, 4, _capi.BATCH_OPTIMIZE, 10, 3, buf.data_ptr())
    assert n == len(raw)
    assert same(dev.match_coverage(labels, tset, device_ptr=buf.data_ptr(), n=n, **kw), want)
    assert same(dev.select_matches(labels, tset, device_ptr=buf.data_ptr(), n=n, min_new=0.5, **kw), want_s)
    assert np.array_equal(np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=MR.MATCH_DTYPE), raw)   # read in place, never written


def test_tensors_the_public_calls_and_match_lists():
    import torch
    import openfdcm_amd as fd
    w, case = G.world("96x80-b0-d30", False), CS.case("96x80-b0-d30")
    kw = dict(radius=3, bin_tolerance=1, min_coverage=0.1, min_new=0.5, min_pixels=2, max_selected=40)
    want_c = cover(w, case, radius=3, bin_tolerance=1, residual=True)
    want_s = select(w, case, **kw)
    assert same(want_s, case.select(**kw)) and len(want_s[0]) > 3
    t = torch.from_numpy(np.array(case.labels)).cuda()
    got = cover(w, case, labels=t, radius=3, bin_tolerance=1, residual=True)
    assert isinstance(got[1], torch.Tensor) and got[1].device == t.device and same((got[0], got[1].cpu().numpy()), want_c)
    got = select(w, case, labels=t, **kw)
    assert isinstance(got[2], torch.Tensor) and same((got[0], got[1], got[2].cpu().numpy()), want_s)
    assert np.array_equal(t.cpu().numpy(), case.labels)                                # read in place, never written
    assert same(w.dev.select_matches(t, w.tset, case.recs, **kw), want_s[:2])          # without a residual: the handle's own plane
    wide = torch.zeros((case.height, case.width + 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        cover(w, case, labels=wide[:, :case.width])
    # the public calls, base 0, on a record array and on a MatchList; a MatchList indexed by the selection is a MatchList
    assert case.base == 0
    ml = fd.MatchList(case.recs)
    assert same(fd.match_coverage(w.dev, case.labels, case.tmpls, ml, radius=3, return_residual=True), want_c)
    assert same((fd.match_coverage(w.dev, case.labels, case.tmpls, case.recs, radius=3),), want_c[:1])
    pub = fd.select_matches(w.dev, case.labels, case.tmpls, ml, return_residual=True, **kw)
    assert same(pub, want_s) and len(fd.select_matches(w.dev, case.labels, case.tmpls, ml, **kw)) == 2
    parts = ml[pub[0]]
    assert isinstance(parts, fd.MatchList) and parts.records().tobytes() == case.recs[pub[0]].tobytes()
    assert same(fd.select_matches(w.dev, case.labels, case.tmpls, case.recs, return_residual=True), case.select())   # the defaults


def test_empty_inputs_and_refused_arguments():
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w, case = G.world("70x37-b5-d30", False), CS.case("70x37-b5-d30")
    none = np.zeros(0, dtype=MR.MATCH_DTYPE)
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts, recs in [(w.dev, w.tset, none), (w.dev, DeviceTemplates([]), case.recs[:3]), (empty_map, w.tset, case.recs[:3])]:
        c, r = fm.match_coverage(w.labels, ts, recs, bin_tolerance=0, residual=True)
        assert c.shape == (len(recs), 2) and np.array_equal(r, w.labels)
        sel, c3, r = fm.select_matches(w.labels, ts, recs, bin_tolerance=0, residual=True)
        assert sel.shape == (0,) and c3.shape == (0, 3) and np.array_equal(r, w.labels)
    bad = case.recs[[20, 21, 36]]                                                     # invalid, invalid, not admissible
    c, r = cover(w, case, bad, residual=True)
    assert np.all(c == -1) and np.array_equal(r, w.labels)
    sel, c3, r = select(w, case, bad)
    assert sel.shape == (0,) and np.array_equal(r, w.labels)
    with pytest.raises(_capi.FdcmError, match=r"bin_tolerance must be in \[0, m / 2\]"):
        cover(w, case, bin_tolerance=w.m // 2 + 1)
    with pytest.raises(_capi.FdcmError, match=r"size must be \(width \+ 2 bx, height \+ 2 by\)"):
        cover(w, case, labels=np.ascontiguousarray(w.labels[:, :-1]))
    many = np.zeros((1 << 16) + 1, dtype=MR.MATCH_DTYPE)
    with pytest.raises(_capi.FdcmError, match="fdcm_matches_detect first"):
        select(w, case, many)
    for kw, msg in [(dict(max_selected=0), "max_selected"), (dict(min_new=1.001), "min_new_permille"), (dict(min_pixels=0), "min_pixels"),
                    (dict(radius=33), "radius")]:
        with pytest.raises(_capi.FdcmError, match=msg):
            select(w, case, **kw)


def _probe(env, *args):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE, *args], capture_output=True, text=True, timeout=240, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("match_coverage_probe ")][-1].split()


def _load_probe():
    spec = __import__("importlib.util").util.spec_from_file_location("match_coverage_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    return probe


def test_switches_and_poison_in_fresh_processes():
    """tools/match_coverage_probe.py in fresh processes, one after another, each under its own time limit; nothing is started
    after a failure (an assertion ends the test).  The digests equal this process's own."""
    digest, admissible, accepted = _load_probe().run()
    assert admissible == 801 and accepted > 10                    # (801: three calls on 267 admissible records, by the referee)
    for env in ({"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_MATCHED_FLAT": "1"}, {"FDCM_FORCE_HOST_BINS": "1"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == admissible and int(line[5]) == accepted, (env, line)


def test_coverage_in_parts_equals_the_uncut_call():
    """2000 records in parts of 600 (FDCM_COVERAGE_PART, read once per process: a fresh one): four parts, the uncut call's bytes."""
    digest, admissible, accepted = _load_probe().run(2000)
    line = _probe({"FDCM_COVERAGE_PART": "600"}, "2000")
    assert line[1] == digest and int(line[3]) == admissible and int(line[5]) == accepted and admissible > 1800, line
