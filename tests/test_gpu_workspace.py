"""GPU tests of the ground every exhaustive call and the seam share: the grow-only workspace search.eval / search.eval_stage
and the volume's allocation.  tools/exhaustive_probe.py runs every call that lays out the workspace on inputs where every
partial write exists (templates of 0, 3, 9 and 70 lines, with and without caps, rotations, grids with partial sub-tiles that
cross the admissible boxes, lists that end early and lists that fill) and digests each call's outputs.  Here:

  1. on the default path the probe's planes are the definitions' (the seam, detect_ref, capped_ref): the other calls are
     functions of these planes, pinned to their referees by the files that came with them;
  2. the digests do not depend on what ran on the handle before: three orders on one handle and a handle per call;
  3. they do not depend on what the workspace and the volume held before the call (FDCM_POISON, words 0 and 1);
  4. nor on the address form of the dense calls (FDCM_EXHAUSTIVE_FLAT), 5. nor on both at once.

The switches are read once per process, so 3 to 5 run the probe in fresh processes.  The tests run in the file's order and
stop at the first process that differs, dies or runs out of time: nothing more is started on a device that has just
misbehaved."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from capped_ref import line_cost_maps
from detect_ref import best_ref, normalised

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "exhaustive_probe.py")
STATE = {"failed": None}  # the first step that differed, died or timed out


def _step(name):
    """The later steps depend on the earlier ones: after a failure they fail at once and start nothing."""
    if STATE["failed"]:
        pytest.fail("not run: '" + STATE["failed"] + "' failed before it")
    STATE["failed"] = name  # until the step says otherwise


def _done():
    STATE["failed"] = None


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("exhaustive_probe", PROBE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def default(probe):
    """The default path, in this process, once: (threshold, digests, counts, outputs) of order "shuffled"."""
    assert not any(k.startswith("FDCM_") for k in os.environ), [k for k in os.environ if k.startswith("FDCM_")]
    thr = probe.threshold()
    digests, counts, outputs = probe.run("shuffled", thr, keep=True)
    print("default run: threshold", float(thr).hex(), "counts", counts)
    return thr, digests, counts, outputs


def test_the_planes_are_the_definitions(probe, default):
    """Step 1.  score_map equals the seam's evaluate at every grid point; the best-map planes equal detect_ref.best_ref of
    the same set's score maps; line_costs equal the cost maps of one-line templates (capped_ref.line_cost_maps)."""
    _step("definitions")
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    thr, digests, counts, out = default
    c = probe.case()
    T = len(c["tmpls"])
    dev = DeviceFeatureMap.build(c["scene"], depth=c["depth"], coeff=c["coeff"], padding=c["padding"], distance=0)
    # the default really is the 32-bit form
    assert dev.depth * dev.device_slice_stride() * 4 < 2 ** 32
    sets = [DeviceTemplates(c["tmpls"]), DeviceTemplates(c["tmpls"], line_caps=c["tau"])]
    # score_map (the set without caps: out["score_map"][0 .. 1]) against the seam
    ev = out["evaluate"]
    inside = outside = 0
    for gi, g in enumerate(c["small"]):
        seam = np.stack(ev[gi * T:(gi + 1) * T]).reshape(T, g[3], g[2])
        got = out["score_map"][gi]
        assert got.shape == seam.shape and got.tobytes() == seam.tobytes()
        inside += int(np.isfinite(got[1:]).sum())
        outside += int(np.isnan(got[1:]).sum())
    print("score_map: admissible points", inside, "others", outside)
    assert inside > 300 and outside > 300  # the grids cross the boxes
    # best map: per set, grid, rotation table and penalty, in _best_map's order
    planes = iter(out["best_score_map"])
    with_pair = without = 0
    winners = set()
    for si, s in enumerate(sets):
        for gi, g in enumerate(c["small"]):
            for rot in (False, True):
                vols = out["rotation_score_map"][si * 2 + gi] if rot else out["score_map"][si * 2 + gi][:, None]
                for penalty, tau in [(None, 1.0), (probe.EXPONENTIAL, 1.5)]:
                    want = best_ref(normalised(vols, s.lengths(), penalty, tau), skip={0})
                    scores, pairs = next(planes), next(planes)
                    assert scores.tobytes() == want[0].tobytes() and np.array_equal(pairs, want[1])
                    winners |= {(si, rot, int(u)) for u in np.unique(pairs[pairs >= 0])}
                    with_pair += int((pairs >= 0).sum())
                    without += int((pairs < 0).sum())
    print("best map: points with a pair", with_pair, "without", without, "winners", sorted(winners))
    assert next(planes, None) is None and with_pair > 1000 and without > 0
    assert len({(rot, u) for _, rot, u in winners}) >= 3  # more than one pair wins somewhere
    # line costs: pose q's floats are the cost maps' values at its grid point, NaN throughout where the pose is inadmissible
    for rot in (False, True):
        cs, pv = (c["cs"], c["piv"]) if rot else (None, None)
        cost, off = out["line_costs"][2 * int(rot)], out["line_costs"][2 * int(rot) + 1]
        capped_cost = out["line_costs"][4 + 2 * int(rot)]
        assert capped_cost.tobytes() == cost.tobytes()  # the costs are uncapped whatever the set
        poses = c["poses"][rot]
        seen = hidden = 0
        for gi, g in enumerate(c["small"]):
            maps, loff = line_cost_maps(dev, c["tmpls"], g, cs, pv)
            maps = maps[:, None] if not rot else maps
            own = out["rotation_score_map"][gi] if rot else out["score_map"][gi][:, None]  # (T, A, ny, nx), the set without caps
            x0, y0, nx, ny, sx, sy = g
            for q, (t, a, x, y) in enumerate(poses):
                i, ri = divmod(int(x) - x0, sx)
                j, rj = divmod(int(y) - y0, sy)
                if ri or rj or not (0 <= i < nx and 0 <= j < ny) or loff[t + 1] == loff[t]:
                    continue
                got = cost[off[q]:off[q + 1]]
                if np.isnan(own[t, a, j, i]):  # the template is not admissible there (a line of its own may be)
                    assert np.isnan(got).all()
                    hidden += 1
                else:
                    assert got.tobytes() == maps[loff[t]:loff[t + 1], a, j, i].tobytes()
                    seen += 1
        print("line costs: poses compared", seen, "inadmissible", hidden)
        assert seen > 300 and (hidden > 0 or not rot)
        assert np.isnan(cost[off[len(poses) - 3]:off[len(poses) - 1]]).all() and off[-1] == off[-2]  # far poses; no lines
    _done()


def test_the_default_run_is_not_vacuous(probe, default):
    _step("conditions")
    thr, digests, counts, out = default
    assert sorted(digests) == sorted(n for n, _ in probe.CALLS)
    assert counts["finite"] > 1000 and counts["nan"] > 1000 and counts["records"] > 1000
    assert counts["short"] >= 1  # a list that ended before its room did
    assert counts["full"] >= 1   # a list of max_detections records
    short = [len(r) for r in out["exhaustive_detect_all_threshold"][0::2]]
    full = [len(r) for r in out["exhaustive_detect_all_inf"][0::2]]
    print("lists at the threshold", short, "at +inf", full)
    assert 0 < short[0] < probe.MAX_DET and full[0] == probe.MAX_DET
    _done()


def test_history_does_not_matter(probe, default):
    """Step 2.  In this process, no switch: the calls in three orders on one handle each, and on a handle per call."""
    _step("history")
    thr, digests, counts, _ = default
    for order in ("listed", "reversed", "fresh"):
        got, cnt, _ = probe.run(order, thr)
        differ = sorted(n for n in digests if got.get(n) != digests[n])
        assert not differ, (order, differ)
        assert cnt == counts
    _done()


def _run_probe(env, thr):
    """A fresh process under the switches of env: ({call: digest}, counts line).  Its own time limit; a failure of any kind
    stays in STATE."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE, "--order", "shuffled", "--threshold", float(thr).hex()], capture_output=True, text=True,
                         timeout=300, env={**clean, **env})
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("exhaustive_probe ")]
    digests = {l[1]: l[2] for l in lines if l[1] != "counts"}
    counts = [l for l in lines if l[1] == "counts"][-1][2:]
    return digests, {k: int(v) for k, v in zip(counts[0::2], counts[1::2])}


def _same_as_default(env, default):
    thr, digests, counts, _ = default
    got, cnt = _run_probe(env, thr)
    print(env, "counts", cnt)
    differ = sorted(n for n in digests if got.get(n) != digests[n])
    assert not differ and sorted(got) == sorted(digests), (env, differ)
    assert cnt == counts


@pytest.mark.parametrize("word", ["0", "1"])
def test_poison_does_not_matter(default, word):
    """Step 3.  The workspace, the staging buffer and the volume's allocation hold the word before every call writes."""
    _step("poison " + word)
    _same_as_default({"FDCM_POISON": word}, default)
    _done()


def test_the_address_form_does_not_matter(default):
    """Step 4.  The 64-bit form of every kernel of the dense calls, k_exhaustive<false, kBest | kMap | kTopK, .> and
    k_line_costs<false> among them."""
    _step("flat")
    _same_as_default({"FDCM_EXHAUSTIVE_FLAT": "1"}, default)
    _done()


def test_poison_and_flat_together(default):
    """Step 5.  The flat kernels clamp where the 32-bit ones get a descriptor's zero."""
    _step("poison 1 and flat")
    _same_as_default({"FDCM_POISON": "1", "FDCM_EXHAUSTIVE_FLAT": "1"}, default)
    _done()
