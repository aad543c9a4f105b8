"""Checks around the shared workspace that need no device: the two test switches are documented where the others are, the
probe (tools/exhaustive_probe.py) reaches every C entry point that reserves search.eval or says why not, and its case and
orders are importable and deterministic."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("exhaustive_probe", os.path.join(ROOT, "tools", "exhaustive_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    return probe


@pytest.fixture(scope="module")
def probe():
    return _load()


def test_switches_are_documented():
    with open(os.path.join(ROOT, "openfdcm_amd", "csrc", "fdcm_internal.h")) as f:
        header = f.read()
    block = header[header.index("the tests' switches"):header.index("const TestSwitches& test_switches();")]
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("## 10. Tools and switches"):design.index("## 11.")]
    for name in ("FDCM_EXHAUSTIVE_FLAT", "FDCM_POISON"):
        assert name in block and name in section
    assert "exhaustive_flat" in block and "poison_word" in block  # TestSwitches carries them
    assert "tools/exhaustive_probe.py" in section
    # the switches the new one leaves alone are still there
    assert "FDCM_WINDOWS_FLAT" in block and "FDCM_MATCHED_FLAT" in block
    # every reserve of the shared workspace goes through the one function
    csrc = os.path.join(ROOT, "openfdcm_amd", "csrc")
    sites = 0
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".cpp", ".h")):
            continue
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        if name != "fdcm_host.cpp":
            assert "eval.reserve(" not in text and "eval_stage.reserve(" not in text, name
        sites += text.count("reserve_eval(fm,")
    assert sites >= 8


def test_probe_reaches_every_call_that_reserves_the_workspace(probe):
    from openfdcm_amd import _capi
    names = [s[0] for s in _capi.SYMBOLS if probe.WORKSPACE_SYMBOL.match(s[0])]
    # the families the pattern is meant to find are found
    for stem in ("fdcm_search_exhaustive", "fdcm_search_exhaustive_windows", "fdcm_search_exhaustive_detect_all_matched", "fdcm_score_map",
                 "fdcm_score_map_rotations", "fdcm_best_map", "fdcm_line_costs", "fdcm_matched_fractions", "fdcm_featuremap_evaluate",
                 "fdcm_featuremap_minmax_translation", "fdcm_featuremap_minmax_translation_batch"):
        assert stem in names
    assert len(names) >= 17
    for name in names:
        assert (name in probe.COVERED) != (name in probe.EXEMPT), name  # one or the other
    for name, reason in probe.EXEMPT.items():
        assert name in names and len(reason) > 20
    assert probe.COVERED <= set(names)
    # what COVERED claims the engine can reach: the binding's name appears in the engine's source
    with open(os.path.join(ROOT, "openfdcm_amd", "engine.py")) as f:
        engine = f.read()
    for name in probe.COVERED:
        assert "lib()." + name + "(" in engine, name


def test_case_and_orders_are_deterministic(probe):
    a, b = probe.case(), _load().case()
    assert a.keys() == b.keys()
    for key in a:
        if key == "tmpls":
            assert [t.shape for t in a[key]] == [(4, 0), (4, 3), (4, 9), (4, 70)]
            assert all(x.tobytes() == y.tobytes() and x.dtype == np.float32 for x, y in zip(a[key], b[key]))
        elif key == "poses":
            assert all(a[key][r].tobytes() == b[key][r].tobytes() and a[key][r].dtype == np.int32 for r in (False, True))
        elif isinstance(a[key], np.ndarray):
            assert a[key].tobytes() == b[key].tobytes()
        else:
            assert a[key] == b[key]
    assert a["small"] == [(-95, -100, 37, 70, 1, 1), (-120, -130, 37, 70, 3, 2)] and a["large"] == (-240, -60, 200, 120, 1, 1)
    assert (a["depth"], a["padding"], a["tau"]) == (12, 1.2, 3.0) and a["cs"].shape == (3, 2)
    # the large grid needs more workspace than any small one: planes of 24000 points against 2590
    assert a["large"][2] * a["large"][3] > 4 * a["small"][0][2] * a["small"][0][3]
    o = probe.orders()
    assert set(o) == {"listed", "reversed", "shuffled"} and o == _load().orders()
    names = [n for n, _ in probe.CALLS]
    assert len(set(names)) == len(names) >= 19 and o["listed"] == names and o["reversed"] == names[::-1]
    assert sorted(o["shuffled"]) == sorted(names) and o["shuffled"] != o["listed"] and o["shuffled"] != o["reversed"]
    assert o["listed"][0].startswith("large")  # the large grid first
    assert probe.MAX_DET == 200
