"""GPU tests of what the build, the reference search, the device tail, scene coverage and the calls without a handle find in
memory they did not write: the grow-only buffers of a handle that lives for hours, re-laid-out at every
change of shape, distance, seed kind or template set, and the per-call scratch of the pixel calls.  tools/build_probe.py runs
a fixed list of cases over every path of these calls (each column-descriptor kernel, a height above 4096, ordered sweeps from
the proxy and from history, handles rebuilt through lines, labels, images, levels, an empty scene and a blank image, searches
with both work lists, short templates, host and device output, the tail, a frame pipeline, the pixel calls, coverage and
selection) and digests what each case returns.  Here:

  1. on the default path every array the probe returns is its referee's, bit for bit: oracle.build and edge_ref.reference_volume
     for volumes, oracle.search for records, fdcm_penalize and a stable sort for the tail, edge_ex_ref, lines_ref, pyramid_ref,
     coverage_ref and select_ref for the pixel calls;
  2. the run took the paths it is there for (the probe's counts);
  3. the digests do not depend on what ran on a handle before: the cases listed, reversed, and a handle per case and step;
  4. they do not depend on what the buffers held before the call (FDCM_POISON, words 0 and 1), and the word reached every
     buffer of FILLED;
  5. nor with the literal sweep, the two-kernel compaction, flat addresses and host bins on top of the word 1.

The switches are read once per process, so 4 and 5 run the probe in fresh processes.  The tests run in the file's order and
stop at the first process that differs, dies or runs out of time: nothing more is started on a device that has just
misbehaved."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import coverage_ref
import edge_ex_ref
import edge_ref
import lines_ref
import pyramid_ref
import select_ref
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "build_probe.py")
STATE = {"failed": None}  # the first step that differed, died or timed out

# The buffers FDCM_POISON fills and the probe's cases use (openfdcm_amd._capi.POISON_BUFFERS names them all): each has a fill
# count above 0 in a process under the switch.  search.bins and its staging exist only where the bins come from the host
# (step 5); search.eval, its staging are tests/test_gpu_workspace.py's.
FILLED = ("vol", "ivol", "bitmap", "coldesc", "colmask", "labels", "edge_parent", "edge_roots", "pyr", "offtab", "stack", "plan",
          "build_stage", "scene", "pairs", "records", "flags", "work", "counter", "out", "search_stage", "cnt", "tail", "tail_out",
          "coverage", "coverage_stage", "pixel_pixels", "pixel_labels", "pixel_keys", "pixel_parent", "pixel_counts", "pixel_comps",
          "pixel_out")
FILLED_WITH_HOST_BINS = ("bins", "bins_stage")
# counts that describe the path, not the inputs: the switches of step 5 change them
PATH_COUNTS = ("order_history", "order_proxy", "compact_one", "compact_two")


def _step(name):
    """The later steps depend on the earlier ones: after a failure they fail at once and start nothing."""
    if STATE["failed"]:
        pytest.fail("not run: '" + STATE["failed"] + "' failed before it")
    STATE["failed"] = name  # until the step says otherwise


def _done():
    STATE["failed"] = None


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("build_probe", PROBE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def default(probe):
    """The default path, in this process, once: (digests, counts, outputs) of order "listed"."""
    assert not any(k.startswith("FDCM_") for k in os.environ), [k for k in os.environ if k.startswith("FDCM_")]
    t0 = time.time()
    digests, counts, outputs = probe.run("listed", keep=True)
    print("default run: %.1f s, counts %s" % (time.time() - t0, counts))
    return digests, counts, outputs


# ---------------------------------------------------------------- the referees, one per spec of the probe
class Referee:
    def __init__(self, probe):
        self.inp = probe.inputs()
        self.probe = probe

    @functools.lru_cache(maxsize=None)
    def labels(self, name, depth, smooth, low, high, min_pixels, level=0):
        img = self.inp["images"][name]
        if level:
            img = pyramid_ref.level_image(img, level)
        return edge_ex_ref.edge_labels(img, depth, smooth, low, high, min_pixels)

    @functools.lru_cache(maxsize=None)
    def lines_map(self, key, depth, distance, stop_after):
        return O.build(self.inp["scenes"][key], depth=depth, coeff=self.probe.COEFF, padding=self.probe.PADDING, distance=distance,
                       nthreads=16, stop_after=stop_after)

    @functools.lru_cache(maxsize=None)
    def pixel_volume(self, lspec, border, depth, distance, stop_after):
        kind, name, level, smooth, low, high, min_pixels = lspec
        return edge_ref.reference_volume(self.labels(name, depth, smooth, low, high, min_pixels, level), border, depth, self.probe.COEFF,
                                         distance, stop_after)

    @functools.lru_cache(maxsize=None)
    def map_of(self, map_spec):
        if map_spec[0] == "lines_volume":
            return self.lines_map(*map_spec[1:])
        keys, vol = self.pixel_volume(*map_spec[1:])
        return O.from_volume(keys, vol, np.float32([map_spec[2], map_spec[2]]))

    @functools.lru_cache(maxsize=None)
    def records(self, map_spec, tkey, scene_key, maxT, maxS, optimizer, batch, base):
        want = np.array(O.search(self.map_of(map_spec), self.inp["tsets"][tkey], self.inp["scenes"][scene_key], maxT, maxS, kind=optimizer,
                                 batch=batch, nthreads=16), copy=True)
        want["tmpl_idx"] += base
        return want

    def topk(self, rspec, k, penalty, tau, lengths):
        from openfdcm_amd import _capi
        rec = np.array(self.records(*rspec[1:]), copy=True)
        base = rspec[-1]
        if penalty is not None:
            rec["tmpl_idx"] -= base
            _capi.check(_capi.lib().fdcm_penalize(penalty, tau, C.c_void_p(rec.ctypes.data), len(rec), _capi.fptr(lengths), len(lengths)))
            rec["tmpl_idx"] += base
        return rec[np.argsort(rec["score"], kind="stable")[:k]]

    @functools.lru_cache(maxsize=None)
    def cover(self, lspec, name):
        lab = self.labels(*lspec[1:])
        h, w = lab.shape
        keys = edge_ref.keys_of(30)
        args = (lab, keys, np.float32([0, 0]), w, h, self.inp["tsets"]["cover"], self.inp["poses"][name])
        counts, residual, _ = coverage_ref.coverage(*args)
        return counts, residual, select_ref.select(*args, min_new=0.3, max_selected=16)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_the_default_run_is_the_definitions(probe, default):
    """Step 1.  Every item of every case against the referee its spec names."""
    _step("definitions")
    from openfdcm_amd.engine import DeviceTemplates
    digests, counts, outputs = default
    ref = Referee(probe)
    lengths = {k: DeviceTemplates(v).lengths() for k, v in ref.inp["tsets"].items()}
    seen = {}
    for case, items in outputs.items():
        for i, (spec, got) in enumerate(items):
            kind = spec[0]
            seen[kind] = seen.get(kind, 0) + 1
            where = (case, i, spec)
            if kind == "lines_volume":
                key, depth, distance, stop = spec[1:]
                if ref.inp["scenes"][key].shape[1] == 0:
                    assert got.size == 0, where
                    continue
                want = ref.lines_map(key, depth, distance, stop).volume()
                assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), where
            elif kind == "pixel_volume":
                want = ref.pixel_volume(*spec[1:])[1]
                assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), where
            elif kind == "records":
                want = ref.records(*spec[1:])
                assert len(got) == len(want) and got.tobytes() == want.tobytes(), (where, len(got), len(want))
            elif kind == "topk":
                rspec, k, penalty, tau = spec[1:]
                assert got.tobytes() == ref.topk(rspec, k, penalty, tau, lengths[rspec[2]]).tobytes(), where
            elif kind == "labels":
                assert _same(got, ref.labels(*spec[1:])), where
            elif kind == "segments":
                want, _ = lines_ref.segments(ref.labels(*spec[1][1:]), len(edge_ref.keys_of(30)), 4, 8, 8)
                assert _same(got, want), (where, got.shape, want.shape)
            elif kind == "pyramid":
                assert _same(got, pyramid_ref.level_image(ref.inp["images"][spec[1]], spec[2])), where
            elif kind.startswith(("coverage_", "select_")):
                counts_w, residual_w, (sel_w, rows_w, sres_w) = ref.cover(spec[1], spec[2])
                want = {"coverage_counts": counts_w, "coverage_residual": residual_w, "select_selected": sel_w, "select_counts": rows_w,
                        "select_residual": sres_w}[kind]
                assert _same(got, want), where
            else:
                raise AssertionError("no referee for " + repr(spec))
    print("items held to their referees:", seen)
    assert set(seen) == {"lines_volume", "pixel_volume", "records", "topk", "labels", "segments", "pyramid", "coverage_counts",
                         "coverage_residual", "select_selected", "select_counts", "select_residual"}
    _done()


def test_the_default_run_is_not_vacuous(probe, default):
    """Step 2.  The paths, from the probe's counts (the probe asserts each build's column-descriptor kernel from the handle's
    geometry itself)."""
    _step("conditions")
    digests, c, outputs = default
    assert sorted(digests) == sorted(n for n, _ in probe.CASES)
    assert FILLED == probe.USED_BUFFERS and FILLED_WITH_HOST_BINS == probe.HOST_BINS_BUFFERS  # what the probe says its cases use
    assert c["short_templates"] > 0                                   # k_pairs wrote -1 slots
    assert c["worklist_block"] > 0 and c["worklist_generic"] > 0      # both work-list forms
    assert c["compact_one"] > 0 and c["compact_two"] == 0             # the one-kernel compaction (the other: step 5)
    assert c["order_proxy"] >= 2 and c["order_history"] >= 2          # both order sources, lines and image
    assert c["steals_kept"] >= 1                                      # a rebuild of the same shape on a balanced handle
    assert c["hw16"] > 0 and c["hw32"] > 0 and c["hw64"] > 0 and c["tall"] >= 2   # every pass-1 kernel; bitmap on the tall ones
    assert c["hysteresis"] >= 3 and c["levels"] >= 3                  # edge_parent / edge_roots and pyr, per distance
    assert c["left_behind"] >= 3                                      # a smaller build on a handle that held a larger one
    assert c["records"] > 10000 and c["segments"] > 10
    sel = [a for s, a in outputs["coverage"] if s[0] == "select_selected"]
    cov = [a for s, a in outputs["coverage"] if s[0] == "coverage_counts"]
    print("selected", [len(a) for a in sel], "explained", [int((a[:, 1] > 0).sum()) for a in cov])
    assert all(len(a) > 0 for a in sel) and all((a[:, 1] > 0).sum() > 3 and (a[:, 0] < 0).sum() >= 2 for a in cov)
    _done()


def test_history_does_not_matter(probe, default):
    """Step 3.  In this process, no switch: the cases reversed on shared handles, and a handle per case and per step."""
    _step("history")
    digests, counts, _ = default
    for order in ("listed", "reversed", "fresh"):
        t0 = time.time()
        got, cnt, _ = probe.run(order)
        print("order %s: %.1f s" % (order, time.time() - t0))
        differ = sorted(n for n in digests if got.get(n) != digests[n])
        assert not differ, (order, differ)
    _done()


def _run_probe(env):
    """A fresh process under the switches of env: ({case: digest}, counts, fills).  Its own time limit; a failure of any kind
    stays in STATE."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    t0 = time.time()
    out = subprocess.run([sys.executable, PROBE, "--order", "listed"], capture_output=True, text=True, timeout=300, env={**clean, **env})
    print(env, "%.1f s" % (time.time() - t0))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("build_probe ")]
    digests = {l[1]: l[2] for l in lines if l[1] not in ("counts", "fills")}
    pairs = lambda name: {k: int(v) for l in lines if l[1] == name for k, v in zip(l[2::2], l[3::2])}
    return digests, pairs("counts"), pairs("fills")


def _same_as_default(env, default, filled, path_counts_may_differ=False):
    digests, counts, _ = default
    got, cnt, fills = _run_probe(env)
    print("counts", cnt, "fills", fills)
    differ = sorted(n for n in digests if got.get(n) != digests[n])
    assert not differ and sorted(got) == sorted(digests), (env, differ)
    skip = PATH_COUNTS if path_counts_may_differ else ()
    assert {k: v for k, v in cnt.items() if k not in skip} == {k: v for k, v in counts.items() if k not in skip}
    missing = [b for b in filled if fills.get(b, 0) == 0]
    assert not missing, ("never filled", missing)
    return cnt


@pytest.mark.parametrize("word", ["0", "1"])
def test_poison_does_not_matter(default, word):
    """Step 4.  Every buffer of FILLED holds the word before the call that uses it writes."""
    _step("poison " + word)
    _same_as_default({"FDCM_POISON": word}, default, FILLED)
    _done()


def test_poison_and_the_other_paths_together(default):
    """Step 5.  The literal sweep, the two-kernel compaction, flat addresses and host bins, each of which leaves results unchanged
    by test_randomised_cases, on top of the word 1."""
    _step("poison 1 and the other paths")
    cnt = _same_as_default({"FDCM_POISON": "1", "FDCM_L2_SWEEP": "literal", "FDCM_SEARCH_COMPACT2": "1", "FDCM_SEARCH_FLAT": "1",
                            "FDCM_FORCE_HOST_BINS": "1"}, default, FILLED + FILLED_WITH_HOST_BINS, path_counts_may_differ=True)
    assert cnt["compact_two"] > 0 and cnt["compact_one"] == 0
    _done()
