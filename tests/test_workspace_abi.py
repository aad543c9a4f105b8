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


def test_switch_comment_struct_and_reader_agree():
    """The switches the header documents are the ones test_switches() reads and TestSwitches carries, and nothing else in the
    library reads the environment; the buffers FDCM_POISON's paragraph promises are the ones the binding names, the header's
    enum lists and tools/build_probe.py claims to use."""
    import re
    from openfdcm_amd import _capi
    csrc = os.path.join(ROOT, "openfdcm_amd", "csrc")
    with open(os.path.join(csrc, "fdcm_internal.h")) as f:
        header = f.read()
    block = header[header.index("the tests' switches"):header.index("const TestSwitches& test_switches();")]
    comment, struct = block[:block.index("struct TestSwitches {")], block[block.index("struct TestSwitches {"):]
    documented = set(re.findall(r"^//   (FDCM_[A-Z0-9_]+)", comment, re.M))
    with open(os.path.join(csrc, "fdcm_host.cpp")) as f:
        host = f.read()
    body = host[host.index("const TestSwitches& test_switches() {"):host.index("static thread_local bool g_no_grow")]
    read = set(re.findall(r'"(FDCM_[A-Z0-9_]+)"', body))
    assert documented == read and len(read) >= 13, (sorted(documented - read), sorted(read - documented))
    members = set()
    for kind, names in re.findall(r"^\s*(bool|int|uint32_t)\s+([^;]+);", re.sub(r"//.*", "", struct), re.M):
        members |= {n.strip() for n in names.split(",")}
    assert members == set(re.findall(r"\br\.(\w+) = ", body)), (members, set(re.findall(r"\br\.(\w+) = ", body)))
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".cpp", ".h")) and name != "fdcm_host.cpp":
            with open(os.path.join(csrc, name)) as f:
                assert "getenv(" not in f.read(), name
    # FDCM_POISON's buffers: the header's enum, the binding's names and the paragraph
    with open(os.path.join(ROOT, "include", "fdcm.h")) as f:
        public = f.read()
    enum = public[public.index("enum fdcm_poison_buffer {"):public.index("FDCM_FILL_BUFFERS")]
    names = [n.lower() for n in re.findall(r"FDCM_FILL_([A-Z_]+)", enum)]
    assert tuple(names) == _capi.POISON_BUFFERS and "fdcm_selftest_poison_fills" in [s[0] for s in _capi.SYMBOLS]
    poison = comment[comment.index("FDCM_POISON="):]
    member = {"vol": "volume", "build_stage": "build.stage", "search_stage": "search.stage", "out": "search.out", "tail": "search.tail",
              "tail_out": "search.tail_out", "eval": "search.eval", "eval_stage": "search.eval_stage", "cnt": " cnt"}
    for n in names:
        assert ("PixelScratch" if n.startswith("pixel_") else member.get(n, n)) in poison, n
    for word in ("sweep.cost_chunks", "sweep.steals_off", "groups", "DESIGN.md"):
        assert word in poison
    spec = importlib.util.spec_from_file_location("build_probe", os.path.join(ROOT, "tools", "build_probe.py"))
    bp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bp)
    assert set(bp.USED_BUFFERS) | set(bp.HOST_BINS_BUFFERS) == set(names) - {"eval", "eval_stage"}
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("## 32."):]
    for word in ("poison_fill", "fdcm_selftest_poison_fills", "tools/build_probe.py", "tests/test_gpu_build_workspace.py", "sweep.steals_off",
                 "sweep.cost_chunks", "groups == (m, W)", "search.out", "PixelScratch", "coverage_stage"):
        assert word in section, word
    assert "tools/build_probe.py" in design[design.index("## 10. Tools and switches"):design.index("## 11.")]
