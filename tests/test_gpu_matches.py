"""GPU tests of the calls on match lists (include/fdcm.h, "Match lists"): fdcm_matches_verify, fdcm_matches_detect and
fdcm_matches_footprints equal the referee (tests/match_ref.py: numpy and Python integers on the volume, nothing from the
kernels) byte for byte -- there is no tolerance to choose; a NaN compares as the one quiet NaN, its payload being no result.
Two maps (a line-built one of about 117 pixels, whose volume is the device's own build, and an adopted 70 x 37 volume that
holds a NaN and an infinity), templates of 0 to 130 lines, four kinds of caps, lists of 1, 255, 256, 257 and 700 records of
every kind match_cases.record_list makes.  Then the rounds across a batch, the three input forms on what search_raw returns,
the section's identities against fdcm_topk, the exhaustive calls and evaluate, two runs, the public calls, the switches
and FDCM_POISON in fresh processes (tools/match_probe.py), and two instances of one part end to end.

fdcm_matches_footprints takes a template handle, which a process without a device cannot make: it is compared with the
referee here and not in test_match_definition.py, as fdcm_templates_footprints is."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases as MC
import match_ref as R
from helpers import ROOT

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "match_probe.py")
MAPS = ("lines", "adopted")


class World:
    def __init__(self, name):
        from openfdcm_amd import synthetic
        from openfdcm_amd.engine import DeviceFeatureMap
        self.name = name
        self.base = 0 if name == "lines" else 5
        self.scene = synthetic.scene(90, 24, 11)
        if name == "lines":
            self.dev = DeviceFeatureMap.build(self.scene, depth=12, coeff=5.0, padding=1.3, distance=0)
            self.keys, self.vol, self.t = self.dev.keys, self.dev.volume(), self.dev.scene_translation
        else:
            self.keys, self.vol, self.t = MC.adopted_volume()
            self.dev = DeviceFeatureMap.from_volume(self.keys, self.vol, self.t)
        self.W, self.H = self.vol.shape[1], self.vol.shape[2]
        self.tmpls = MC.template_set()
        self.recs = MC.record_list(77, self.W, self.H, self.t, self.tmpls, 700, self.base)
        self.lengths = R.template_lengths(self.tmpls)
        self._tsets, self._ref = {}, {}

    def caps(self, kind):
        return MC.caps_of(self.tmpls, kind)

    def tset(self, kind="none"):
        from openfdcm_amd.engine import DeviceTemplates
        if kind not in self._tsets:
            self._tsets[kind] = DeviceTemplates(self.tmpls, line_caps=self.caps(kind))
        return self._tsets[kind]

    def ref(self, kind="none"):
        """The referee's verify of the 700 records, computed once per kind of caps."""
        if kind not in self._ref:
            self._ref[kind] = R.verify(self.vol, self.keys, self.t, self.tmpls, self.recs, self.base, self.caps(kind))
        return self._ref[kind]

    def detect_ref(self, kind, n, **kw):
        return R.detect(self.vol, self.keys, self.t, self.tmpls, self.recs[:n], self.base, caps=self.caps(kind),
                        verified=tuple(a[:n] for a in self.ref(kind)), **kw)


@functools.lru_cache(maxsize=None)
def world(name):
    return World(name)


def same_detection(got, want):
    return (MC.same_records(got[0], want[0]) and got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
            and got[2].dtype == np.int32 and got[2].shape == want[2].shape and np.array_equal(got[2], want[2]) and MC.same_floats(got[3], want[3]))


def run_detect(w, kind, n, permille=300, den=None, penalty=None, tau=1.0, **kw):
    """(device, referee) of one detect call on the first n records."""
    got = w.dev.detect_matches(w.tset(kind), w.recs[:n], overlap_permille=permille, penalty=penalty, tau=tau, tmpl_index_base=w.base,
                               indices=True, boxes=True, matched=True, **kw)
    want = w.detect_ref(kind, n, permille=permille, den=None if penalty is None else R.denominators(w.tmpls, penalty, tau), **kw)
    return got, want


@pytest.mark.parametrize("kind", MC.CAPS)
@pytest.mark.parametrize("name", MAPS)
def test_verify_equals_the_referee(name, kind):
    w = world(name)
    s, f, c, ml, adm = w.ref(kind)
    assert adm.sum() > 350 and (~adm).sum() > 60
    for n in MC.LENGTHS:
        gs, gf, gc = w.dev.verify_matches(w.tset(kind), w.recs[:n], tmpl_index_base=w.base)
        assert MC.same_floats(gs, s[:n]) and MC.same_floats(gf, f[:n]) and MC.same_floats(gc, c[:n]), (n, np.flatnonzero(MC.canon(gs) != MC.canon(s[:n]))[:5])
    if kind == "none":      # a record that is not valid or not admissible is NaN throughout; a template without lines scores +0
        bad = ~adm
        assert np.isnan(gs[bad]).all() and np.isnan(gf[bad]).all() and np.isnan(gc[bad]).all()
        empty = adm & (w.recs["tmpl_idx"] - w.base == 0)
        assert empty.any() and np.all(gs[empty].view(np.uint32) == 0) and np.all(gf[empty] == 1)
    if name == "adopted" and kind == "none":
        assert np.isinf(gs[adm]).any() and np.isnan(gs[adm]).any()     # the volume's infinity and NaN are reached


@pytest.mark.parametrize("kind", MC.CAPS)
@pytest.mark.parametrize("name", MAPS)
def test_detect_equals_the_referee(name, kind):
    w = world(name)
    kept = 0
    for n in MC.LENGTHS:
        for kw in (dict(penalty=0), dict(permille=0, max_score=25.0, margin=3), dict(permille=500, penalty=1, tau=0.5, min_matched=0.5, rescore=True,
                                                                                     max_score=40.0),
                   dict(permille=1000, max_detections=4096, rescore=True), dict(permille=150, min_matched=1.0)):
            got, want = run_detect(w, kind, n, **kw)
            assert same_detection(got, want), (n, kw, len(got[0]), len(want[0]), got[1][:6], want[1][:6])
            kept += len(want[0])
    assert kept > 200


@pytest.mark.parametrize("max_detections", [1, 64, 65, 200])
def test_the_rounds_cross_a_batch(max_detections):
    w = world("lines")
    got, want = run_detect(w, "none", 700, permille=1000, max_detections=max_detections)
    assert len(want[0]) == max_detections and same_detection(got, want)
    got, want = run_detect(w, "scalar", 700, permille=300, penalty=0, max_detections=max_detections)
    assert same_detection(got, want)


@functools.lru_cache(maxsize=None)
def searched():
    """What search_raw returns on the line-built map, with base 7, and the referee's verify of it."""
    from openfdcm_amd.engine import search_raw
    w = world("lines")
    raw = search_raw(w.dev, w.tset(), w.scene, 4, 4, 1, 10, 7)
    return raw, R.verify(w.vol, w.keys, w.t, w.tmpls, raw, 7)


def test_the_three_input_forms_on_search_records():
    import torch
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import search_into
    w = world("lines")
    raw, ref = searched()
    assert len(raw) > 100 and ref[4].sum() > 50
    den = R.denominators(w.tmpls, 0)
    want_v = ref[:3]
    want_d = R.detect(w.vol, w.keys, w.t, w.tmpls, raw, 7, permille=300, den=den, verified=ref)
    assert 0 < len(want_d[0]) < len(raw)
    kw = dict(overlap_permille=300, penalty=0, tmpl_index_base=7, indices=True, boxes=True, matched=True)
    # the last search (search_raw just ran in searched(), or runs again here), host records, device records
    from openfdcm_amd.engine import search_raw
    assert MC.same_records(search_raw(w.dev, w.tset(), w.scene, 4, 4, 1, 10, 7), raw)
    forms = [dict(matches=None), dict(matches=raw)]
    buf = torch.empty(w.tset().capacity(w.scene.shape[1], 4, 4) * 32, dtype=torch.uint8, device="cuda")
    for form in forms:
        got = w.dev.verify_matches(w.tset(), tmpl_index_base=7, **form)
        assert all(MC.same_floats(g, v) for g, v in zip(got, want_v)), form.keys()
        assert same_detection(w.dev.detect_matches(w.tset(), **form, **kw), want_d)
    n = search_into(w.dev, w.tset(), w.scene, 4, 4, _capi.BATCH_OPTIMIZE, 10, 7, buf.data_ptr())
    assert n == len(raw)
    got = w.dev.verify_matches(w.tset(), tmpl_index_base=7, device_ptr=buf.data_ptr(), n=n)
    assert all(MC.same_floats(g, v) for g, v in zip(got, want_v))
    assert same_detection(w.dev.detect_matches(w.tset(), device_ptr=buf.data_ptr(), n=n, **kw), want_d)
    assert np.array_equal(np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=R.MATCH_DTYPE), raw)   # read in place, never written


@pytest.mark.parametrize("penalty,tau", [(None, 1.0), (0, 1.0), (1, 1.5)])
def test_identity_1_everything_kept_is_topk(penalty, tau):
    """overlap 1000, no threshold, no gate, rescore 0 on a list whose records are all candidates: fdcm_topk with k = n."""
    from openfdcm_amd.engine import search_raw, topk
    w = world("lines")
    raw, ref = searched()
    cand = raw[ref[4] & ~np.isnan(raw["score"]) & ~np.signbit(raw["score"])]
    cand = np.concatenate([cand, cand[:40]])                       # ties in positional order
    assert len(cand) > 64
    buf_rec = np.ascontiguousarray(cand)
    import torch
    buf = torch.from_numpy(buf_rec.view(np.uint8).copy()).cuda()
    want = topk(w.dev, w.tset(), len(cand), penalty, tau, tmpl_index_base=7, device_ptr=buf.data_ptr(), n=len(cand))
    got = w.dev.detect_matches(w.tset(), cand, overlap_permille=1000, max_detections=4096, penalty=penalty, tau=tau, tmpl_index_base=7)
    assert len(got) == len(cand) and got.tobytes() == want.tobytes()
    got = w.dev.detect_matches(w.tset(), device_ptr=buf.data_ptr(), n=len(cand), overlap_permille=1000, max_detections=4096, penalty=penalty,
                               tau=tau, tmpl_index_base=7)
    assert got.tobytes() == want.tobytes()


def test_identity_5_integer_translations_are_the_exhaustive_calls():
    from openfdcm_amd.engine import DeviceTemplates
    w = world("adopted")        # its translation (3.5, -2.25) and integer coordinates keep every sum exact, in either order
    tm = MC.template_set(9, integer=True)
    rng = np.random.default_rng(3)
    n = 120
    tr = np.stack([rng.integers(-10, w.W - 10, size=n), rng.integers(-10, w.H - 10, size=n)], axis=1)
    ti = rng.integers(0, len(tm), size=n)
    recs = R.records(ti, np.zeros(n), [[1, 0, x, 0, 1, y] for x, y in tr])
    poses = np.stack([ti, np.zeros(n, dtype=np.int64), tr[:, 0], tr[:, 1]], axis=1).astype(np.int32)
    for caps in (None, MC.caps_of(tm, "mixed")):
        tset = DeviceTemplates(tm, line_caps=caps)
        s, f, c = w.dev.verify_matches(tset, recs)
        flat, off = w.dev.line_costs(tset, poses)
        for q in range(n):
            k = off[q + 1] - off[q]
            assert MC.same_floats(c[q, :k], flat[off[q]:off[q + 1]]) and np.isnan(c[q, k:]).all()
        assert MC.same_floats(f, w.dev.matched_fractions(tset, poses))
        jobs = np.stack([ti, np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64), tr[:, 0], tr[:, 1], np.ones(n, dtype=np.int64),
                         np.ones(n, dtype=np.int64)], axis=1).astype(np.int32)
        win, offs = w.dev.exhaustive_window_search(tset, jobs, k=1)
        for q in range(n):
            if offs[q + 1] > offs[q]:
                assert win["score"][offs[q]].tobytes() == s[q].tobytes()
            elif tm[ti[q]].shape[1]:            # (the windows' call has no record for a template without lines; s is +0)
                assert np.isnan(s[q])
            else:
                assert s[q].tobytes() == np.float32(0).tobytes()
        assert (~np.isnan(s)).sum() > 40 and np.isnan(s).sum() > 10


def test_the_score_is_evaluate_of_the_posed_lines():
    w = world("adopted")
    s = w.dev.verify_matches(w.tset(), w.recs, tmpl_index_base=w.base)[0]
    costs = w.dev.verify_matches(w.tset(), w.recs, tmpl_index_base=w.base)[2]
    posed = [R.posed(w.tmpls, r, w.base) for r in w.recs]
    valid = [j for j, p in enumerate(posed) if p is not None]
    with np.errstate(all="ignore"):
        got = w.dev.evaluate([posed[j] for j in valid], [np.zeros((1, 2), dtype=np.float32)] * len(valid))
    nonempty = [j for j, g in zip(valid, got) if posed[j].shape[1]]
    assert MC.same_floats(np.array([g[0] for j, g in zip(valid, got) if posed[j].shape[1]], dtype=np.float32), s[nonempty])
    # a line's cost is evaluate of the one-line template
    j = next(j for j in nonempty if posed[j].shape[1] == 9 and not np.isnan(s[j]))
    one = w.dev.evaluate([posed[j][:, i:i + 1] for i in range(9)], [np.zeros((1, 2), dtype=np.float32)] * 9)
    assert MC.same_floats(np.array([o[0] for o in one], dtype=np.float32), costs[j, :9])


def test_footprints_equal_the_referee_and_the_boxes_of_the_detect_call():
    from openfdcm_amd.engine import match_footprints
    w = world("adopted")
    for margin in (0, 3, 4096):
        want = R.footprints(w.tmpls, w.recs, w.base, margin)
        got = match_footprints(w.tset(), w.recs, margin, tmpl_index_base=w.base)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        res = w.dev.detect_matches(w.tset(), w.recs, overlap_permille=1000, max_detections=4096, margin=margin, tmpl_index_base=w.base,
                                   indices=True, boxes=True)
        assert np.array_equal(res[2], want[res[1]])
    inf = np.array(w.recs[:4])
    inf["tmpl_idx"] = w.base + 3
    inf["transform"][:, 2] = [np.inf, -np.inf, 1e30, np.nan]
    got = match_footprints(w.tset(), inf, 2, tmpl_index_base=w.base)
    assert np.array_equal(got, R.footprints(w.tmpls, inf, w.base, 2)) and got[0, 0] == 1 << 25 and got[1, 2] == -(1 << 25) and tuple(got[3]) == (0, 0, -1, -1)


def test_two_runs_and_the_public_calls():
    import openfdcm_amd as fd
    w = world("lines")
    kw = dict(overlap_permille=300, penalty=0, min_matched=0.3, rescore=True, indices=True, boxes=True, matched=True)
    first = w.dev.detect_matches(w.tset("scalar"), w.recs, **kw)
    v1 = w.dev.verify_matches(w.tset("scalar"), w.recs)
    for _ in range(2):
        again = w.dev.detect_matches(w.tset("scalar"), w.recs, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(v1, w.dev.verify_matches(w.tset("scalar"), w.recs)))
    caps = w.caps("scalar")
    pub = fd.detect_matches(w.dev, w.tmpls, fd.MatchList(w.recs), overlap=0.3, penalty=fd.DefaultPenalty(), line_caps=caps, min_matched=0.3,
                            rescore=True, return_indices=True, return_boxes=True, return_matched=True)
    assert isinstance(pub[0], fd.MatchList) and pub[0].records().tobytes() == first[0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pub[1:], first[1:]))
    one = fd.detect_matches(w.dev, w.tmpls, w.recs, penalty=fd.DefaultPenalty(), line_caps=caps, min_matched=0.3, rescore=True)
    assert isinstance(one, fd.MatchList) and one.records().tobytes() == first[0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fd.verify_matches(w.dev, w.tmpls, w.recs, line_caps=caps), v1))
    assert np.array_equal(fd.match_footprints(w.tmpls, w.recs, margin=2), R.footprints(w.tmpls, w.recs, 0, 2))


def test_empty_inputs_and_refused_arguments():
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates, match_footprints
    w = world("adopted")
    none = np.zeros(0, dtype=R.MATCH_DTYPE)
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts, recs in [(w.dev, w.tset(), none), (w.dev, DeviceTemplates([]), w.recs[:5]), (empty_map, w.tset(), w.recs[:5])]:
        res = fm.detect_matches(ts, recs, indices=True, boxes=True, matched=True)
        assert res[0].shape == (0,) and res[0].dtype == R.MATCH_DTYPE and res[1].shape == (0,) and res[2].shape == (0, 4) and res[3].shape == (0,)
        s, f, c = fm.verify_matches(ts, recs)
        assert np.isnan(s).all() and np.isnan(f).all() and np.isnan(c).all()       # nothing is written: the binding's own NaN
    assert match_footprints(w.tset(), none).shape == (0, 4)
    for kw, msg in [(dict(max_detections=0), "max_detections"), (dict(max_detections=4097), "max_detections"), (dict(overlap_permille=1001), "overlap_permille"),
                    (dict(margin=-1), "margin"), (dict(max_score=-1.0), "max_score"), (dict(max_score=float("nan")), "max_score"),
                    (dict(min_matched=1.5), "min_matched"), (dict(penalty=7), "unknown penalty"), (dict(tau=float("inf")), "tau")]:
        with pytest.raises(_capi.FdcmError, match=msg):
            w.dev.detect_matches(w.tset(), w.recs, **kw)
    with pytest.raises(ValueError, match="match records"):
        w.dev.detect_matches(w.tset(), np.zeros(3, dtype=np.float32))


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=240, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("match_probe ")][-1].split()


def test_switches_and_poison_in_fresh_processes():
    """tools/match_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after a
    failure (an assertion ends the test).  The digests equal this process's own."""
    spec = __import__("importlib.util").util.spec_from_file_location("match_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, values, kept = probe.run()
    assert values > 800 and kept > 100
    for env in ({"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_MATCHED_FLAT": "1"}, {"FDCM_FORCE_HOST_BINS": "1"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == values and int(line[5]) == kept, (env, line)


def test_end_to_end_two_instances_of_one_part():
    """Two instances of one polygon part in a scene: search -> detect_matches between the true poses' q and the best junk
    leaves exactly two records, one per instance; the device equals the referee."""
    import openfdcm_amd as fd
    import match_scene as MS
    scene, tmpls, centres = MS.two_parts()
    fm = fd.build_cpu_featuremap(scene, fd.Dt3CpuParameters(depth=30, dt3Coeff=5.0, padding=2.2))
    matches = fd.search(fd.DefaultMatch(), fd.DefaultSearch(MS.MAX_TMPL, MS.MAX_SCENE), fd.BatchOptimize(10), fm, tmpls, scene)
    dev = fm._fm
    assert len(matches) > 20
    got = fd.detect_matches(fm, tmpls, matches, max_score=MS.MAX_SCORE, overlap=0.3, penalty=fd.DefaultPenalty(), return_indices=True,
                            return_boxes=True, return_matched=True)
    want = R.detect(dev.volume(), dev.keys, dev.scene_translation, tmpls, matches.records(), 0, max_score=MS.MAX_SCORE, permille=300,
                    den=R.denominators(tmpls, 0))
    assert same_detection((got[0].records(), *got[1:]), want)
    assert len(got[0]) == 2
    found = sorted(MS.centre_of(tmpls[m.tmpl_idx], m.transform) for m in got[0])
    assert all(np.hypot(f[0] - c[0], f[1] - c[1]) < 3.0 for f, c in zip(found, sorted(centres)))
    same = fd.detect_matches(fm, tmpls, None, max_score=MS.MAX_SCORE, overlap=0.3, penalty=fd.DefaultPenalty())   # the last search
    assert same.records().tobytes() == got[0].records().tobytes()
