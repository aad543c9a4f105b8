"""GPU tests of the pose fit of match records (include/fdcm.h, "Match lists: pose fit"): the records, the info rows and the rms
values of fdcm_matches_fit equal the referee's (tests/fit_ref.py: Python integers and float64 scalars, nothing from the
kernel) byte for byte -- there is no tolerance to choose -- on the 300 records of fit_cases.py: 96 x 80 labels at border 0
and 5, depth 30 and 6, templates of 0, 1, 3, 64, 65 and 257 lines, windows of one strip and of several, radius 0, 1, 3 and 32,
tolerance 0, 1 and m / 2, 1, 2 and 8 iterations, with and without damping.  Then lists of 1 .. 300 records, the three record
forms on what a real search returns with labels as array and as tensor, output to a device buffer and in place, records
that are invalid or outside the map, empty inputs, the switches in fresh processes (tools/fit_probe.py: FDCM_POISON, the
host's bins, FDCM_COVERAGE_PART forcing several parts), and one planted scene end to end through build_labels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as FR
import match_ref as MR
import select_cases as SC
from helpers import ROOT

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "fit_probe.py")
_DEV = {}


def device(name):
    """(feature map, template set) of a world of fit_cases, built once."""
    if name not in _DEV:
        from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
        w = FC.world(name)
        dev = DeviceFeatureMap.build_labels(w.labels, border=w.border, depth=w.depth)
        assert np.array_equal(dev.keys, w.keys) and (dev.width, dev.height) == (w.W, w.H)
        _DEV[name] = (dev, DeviceTemplates(w.tmpls))
    return _DEV[name]


def same(got, want):
    return all(np.asarray(g).dtype == v.dtype and np.asarray(g).shape == v.shape and np.asarray(g).tobytes() == v.tobytes()
               for g, v in zip(got, want))


def fit(name, recs=None, labels=None, **kw):
    w = FC.world(name)
    dev, tset = device(name)
    return dev.fit_matches(w.labels if labels is None else labels, tset, w.recs if recs is None else recs, tmpl_index_base=w.base,
                           info=True, rms=True, **kw)


def first_difference(got, want):
    bad = [np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(g, v)]) for g, v in zip(got, want)]
    j = min((int(b[0]) for b in bad if len(b)), default=None)
    return None if j is None else (j, [int(len(b)) for b in bad], got[0][j], want[0][j], got[1][j], want[1][j], got[2][j], want[2][j])


@pytest.mark.parametrize("par", FC.PARAMS, ids=lambda p: "r%d-t%s-i%d-d%g" % p)
@pytest.mark.parametrize("name", list(FC.WORLDS))
def test_records_info_and_rms_equal_the_referee(name, par):
    w = FC.world(name)
    want = w.ref(*par)
    got = fit(name, **w.kw(*par))
    assert same(got, want), first_difference(got, want)
    lines = np.array([w.tmpls[t].shape[1] if 0 <= t < len(w.tmpls) else -1 for t in w.recs["tmpl_idx"].astype(np.int64) - w.base])
    assert set(lines.tolist()) == {-1, 0, 1, 3, 64, 65, 257} and len(w.recs) == 300
    status = want[1][:, 0]
    assert (status == -1).sum() >= 20 and (status == 1).sum() >= 1 and (status >= 0).sum() >= 200
    if par[2] > 1 and par[0] > 0:
        assert np.any(want[1][:, 1] > 1) and np.any(want[0]["transform"] != w.recs["transform"])
        assert np.any(want[1][lines == 257, 1] > 0) and np.any(want[1][lines == 64, 1] > 0)    # both sides of the LDS chunk step


def test_the_cases_hold_every_status_and_strip_count():
    """What keeps the comparison above from hiding a failure, on the referee's results."""
    from nms_ref import box_of_lines
    seen = set()
    for name in FC.WORLDS:
        w = FC.world(name)
        for par in FC.PARAMS:
            seen |= set(w.ref(*par)[1][:, 0].tolist())
        area = []
        for r in w.recs:
            p = MR.posed(w.tmpls, r, w.base)
            if p is not None and p.shape[1] and np.all(np.isfinite(p)):
                x0, y0, x1, y1 = (int(v) for v in box_of_lines(p, 3))
                area.append(max(0, min(w.width - 1, x1) - max(0, x0) + 1) * max(0, min(w.height - 1, y1) - max(0, y0) + 1))
        area = np.array(area)
        assert (area > 2048).sum() >= 20 and ((area > 0) & (area <= 2048)).sum() >= 100
    assert seen == {-1, 0, 1, 2, 3, 4}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 300])
def test_lists_of_1_to_300_records(n):
    """A prefix of the list is the prefix of the result: records do not see each other."""
    for name in FC.WORLDS:
        w = FC.world(name)
        want = tuple(a[:n] for a in w.ref(3, 1, 2, 0.0))
        got = fit(name, recs=w.recs[:n], **w.kw(3, 1, 2, 0.0))
        assert same(got, want), first_difference(got, want)


def test_two_runs_a_permutation_and_the_public_call():
    import openfdcm_amd as fd
    w = FC.world("b0-d30")
    dev, _ = device("b0-d30")
    kw = w.kw(1, None, 8)
    want = w.ref(1, None, 8)
    for _ in range(2):
        assert same(fit("b0-d30", **kw), want)
    perm = np.random.default_rng(4).permutation(len(w.recs))
    assert same(fit("b0-d30", recs=w.recs[perm], **kw), tuple(a[perm] for a in want))
    assert w.base == 0
    pub = fd.fit_matches(dev, w.labels, w.tmpls, fd.MatchList(w.recs), return_info=True, return_rms=True, **kw)
    assert isinstance(pub[0], fd.MatchList) and same((pub[0].records(), pub[1], pub[2]), want)
    only = fd.fit_matches(dev, w.labels, w.tmpls, w.recs, **kw)
    assert isinstance(only, fd.MatchList) and only.records().tobytes() == want[0].tobytes()
    defaults = fd.fit_matches(dev, w.labels, w.tmpls, w.recs, return_info=True, return_rms=True)
    ref = FR.fit(w.labels, w.keys, w.T, w.W, w.H, w.tmpls, w.recs)
    assert same((defaults[0].records(), defaults[1], defaults[2]), ref)


def test_the_record_forms_the_label_forms_and_the_output_forms():
    import torch
    import openfdcm_amd as fd
    import test_gpu_coverage as G
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
    kw = dict(radius=3, bin_tolerance=1, iterations=2, tmpl_index_base=3, info=True, rms=True)
    want = FR.fit(labels, dev.keys, (0, 0), dev.width, dev.height, tmpls, raw, 3, radius=3, bin_tolerance=1, iterations=2)
    assert (want[1][:, 0] == 0).sum() > 10 and np.any(want[0]["transform"] != raw["transform"])
    on_dev = torch.from_numpy(np.array(labels)).cuda()
    for lab in (labels, on_dev):
        for form in (dict(matches=None), dict(matches=raw)):       # the last search, host records
            got = dev.fit_matches(lab, tset, **form, **kw)
            assert same(got, want), (form.keys(), first_difference(got, want))
    assert np.array_equal(on_dev.cpu().numpy(), labels)                                     # read in place, never written
    buf = torch.empty(tset.capacity(scene.shape[1], 4, 4) * 32, dtype=torch.uint8, device="cuda")
    n = search_into(dev, tset, scene, 4, 4, _capi.BATCH_OPTIMIZE, 10, 3, buf.data_ptr())
    assert n == len(raw)
    assert same(dev.fit_matches(on_dev, tset, device_ptr=buf.data_ptr(), n=n, **kw), want)  # device records, host output
    assert np.array_equal(np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=MR.MATCH_DTYPE), raw)   # read in place, not written
    other = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    none, info, rms = dev.fit_matches(labels, tset, raw, out_device_ptr=other.data_ptr(), **kw)            # host records, device output
    assert none is None and same((np.frombuffer(other.cpu().numpy().tobytes(), dtype=MR.MATCH_DTYPE), info, rms), want)
    none, info, rms = dev.fit_matches(on_dev, tset, device_ptr=buf.data_ptr(), n=n, out_device_ptr=buf.data_ptr(), **kw)   # in place
    fitted = np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=MR.MATCH_DTYPE)
    assert none is None and same((fitted, info, rms), want)
    # the fitted device buffer goes straight on to detect_matches, rescored
    dk = dict(overlap_permille=300, tmpl_index_base=3, rescore=True, indices=True)
    a = dev.detect_matches(tset, device_ptr=buf.data_ptr(), n=n, **dk)
    b = dev.detect_matches(tset, want[0], **dk)
    assert len(b[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_invalid_records_empty_inputs_and_refusals():
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = FC.world("b5-d6")
    dev, tset = device("b5-d6")
    status = w.ref(3, 1, 2, 0.0)[1][:, 0]
    bad = w.recs[status == -1]
    out, info, rms = fit("b5-d6", recs=bad)                        # invalid, NaN, outside the map: untouched
    assert len(bad) >= 20 and out.tobytes() == bad.tobytes() and np.all(info == (-1, 0, 0, 0)) and np.isnan(rms).all()
    none = np.zeros(0, dtype=MR.MATCH_DTYPE)
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts, rr in [(dev, tset, none), (dev, DeviceTemplates([]), w.recs[:5]), (empty_map, tset, w.recs[:5])]:
        out, info, rms = fm.fit_matches(w.labels, ts, rr, bin_tolerance=0, info=True, rms=True)
        assert out.tobytes() == rr.tobytes() and info.shape == (len(rr), 4) and np.all(info == (-1, 0, 0, 0)) and np.isnan(rms).all()
    with pytest.raises(_capi.FdcmError, match=r"bin_tolerance must be in \[0, m / 2\]"):
        fit("b5-d6", bin_tolerance=w.m // 2 + 1)
    with pytest.raises(_capi.FdcmError, match=r"size must be \(width \+ 2 bx, height \+ 2 by\)"):
        fit("b5-d6", labels=np.ascontiguousarray(w.labels[:, :-1]))
    for kw, msg in [(dict(iterations=9), "iterations"), (dict(min_pixels=2), "min_pixels"), (dict(damping=-1.0), "damping"),
                    (dict(max_angle=float("nan")), "max_angle"), (dict(radius=33), "radius")]:
        with pytest.raises(_capi.FdcmError, match=msg):
            fit("b5-d6", **kw)


def _probe(env, *args):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE, *args], capture_output=True, text=True, timeout=240, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("fit_probe ")][-1].split()


def test_switches_poison_and_parts_in_fresh_processes():
    """tools/fit_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after a
    failure (an assertion ends the test).  300 records in parts of 90 (FDCM_COVERAGE_PART, read once per process) are four
    parts.  The digests equal this process's own, and its counts are the referee's."""
    spec = __import__("importlib.util").util.spec_from_file_location("fit_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, stepped, stopped = probe.run()
    w = FC.world(probe.WORLD)
    infos = [w.ref(*FC.PARAMS[k])[1] for k in probe.PARAMS]
    assert stepped == sum(int((i[:, 1] > 0).sum()) for i in infos) > 300 and stopped == sum(int((i[:, 0] > 0).sum()) for i in infos) > 100
    for env in ({"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_FORCE_HOST_BINS": "1"}, {"FDCM_COVERAGE_PART": "90"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == stepped and int(line[5]) == stopped, (env, line)


def test_a_planted_scene_end_to_end():
    """Case 1 of fit_cases.planted (the referee's worst) through build_labels and the public call: the referee's bytes, and
    the bound test_fit_scene.py holds the referee to."""
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    cases, keys, tmpls = FC.planted()
    labels, true, start = cases[1]
    dev = DeviceFeatureMap.build_labels(labels, border=0, depth=FC.DEPTH)
    assert np.array_equal(dev.keys, keys)
    got = fd.fit_matches(dev, labels, tmpls, start, return_info=True, return_rms=True, **FC.FIT)
    want = FC.planted_fit(1)
    assert same((got[0].records(), got[1], got[2]), want)
    before, after = FC.error(start["transform"][0], true), FC.error(got[0].records()["transform"][0], true)
    assert after <= FC.MAX_ERROR and after <= FC.MAX_SHARE * before, (before, after)
