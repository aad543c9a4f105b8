"""The line-walk search on volumes designed to walk the optimiser to the map's edge (tests/walk_cases.py).

Every search test elsewhere compares the search kernel with the oracle on volumes built from scenes, where a descent ends
after a batch or two.  Here the volume decides the walk, for DefaultOptimize, IndulgentOptimize(3) and BatchOptimize at
every batch size where the kernel's structure changes (one gather round or two at 15 / 16, the 32-slot rounds, the pieces
of 64 of the reduction over a batch, batches of more than a whole walk):

  ramp      the walk ends at the last admissible multiplier of minmaxTranslation, through several windows of scores
  plateau   the walk goes through the whole range in both directions on equal scores; multiplier 0 must win
  valley    the walk stops inside the range, at every position of a batch as the valley moves pixel by pixel

The oracle half asserts, from the oracle's records and statistics alone, that the inputs force those paths (the
witnesses); it runs without a GPU.  The device half asserts that the library's records are the oracle's byte for byte on
the same inputs, and that fdcm_search_timing's counts are the rule's.
"""
import numpy as np
import pytest

import walk_cases as wc
from oracle import oracle as O

BACKENDS = [pytest.param("oracle", id="oracle"), pytest.param("device", id="device", marks=pytest.mark.gpu)]
OPTS = list(wc.OPTIMISERS)
SMALL = [o for o in OPTS if wc.OPTIMISERS[o][0] != O.INDULGENT_OPTIMIZE and wc.OPTIMISERS[o][1] <= 16]   # B <= 16
SWEEP_COUNTS = (4, 9, 65)


def _search(backend, name, opt, n):
    """The oracle's (records, stats), every candidate valid (witness 5); on the device backend the library is held to
    them first."""
    if backend == "device":
        wc.check_device(name, opt, n)
    rec, stats = wc.oracle_search(name, opt, n)
    assert len(rec) == stats[1] == 2 * min(n, 4) * 4 * len(wc.templates(n)), (name, opt, n, len(rec), stats)
    return rec, stats


def _assert_windows_refilled(name, opt, n, stats):
    """Witness 2: 60 evaluations per candidate are four windows of 15: no candidate average below that without a second,
    third and fourth call of the kernel's score_range from inside the replay."""
    per_candidate = wc.evaluations(stats, n) / stats[1]
    assert per_candidate >= 60, (name, opt, n, per_candidate)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("name", ["ramp", "ramp-t"])
def test_ramp_walks_to_the_last_multiplier(backend, opt, name):
    """Witness 1: on the ramp at least 95 % of the records put the moved template's largest coordinate within two pixels
    of the map's far edge, whatever the optimiser; for B <= 16 through refilled windows."""
    for n in wc.LINE_COUNTS:
        rec, stats = _search(backend, name, opt, n)
        at_edge = wc.moved_max(name, rec, n) >= wc.SIZE - 2
        assert at_edge.mean() >= 0.95, (name, opt, n, at_edge.mean())
        if opt in SMALL:
            _assert_windows_refilled(name, opt, n, stats)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("name", ["plateau", "plateau-t"])
def test_plateau_keeps_multiplier_zero(backend, opt, name):
    """Witness 3: on equal scores every optimiser and batch size walks the whole range (as many evaluations as
    DefaultOptimize, which stops at nothing but a higher score) and returns the same records: the alignment itself, whose
    score is O.evaluate of the aligned template at translation 0."""
    fm = wc.oracle_map(name)
    for n in wc.LINE_COUNTS:
        rec, stats = _search(backend, name, opt, n)
        base, base_stats = wc.oracle_search(name, "default", n)
        wc.same_records(rec, base, f"{name} {opt} {n} lines against DefaultOptimize")
        assert stats[0] == base_stats[0], (name, opt, n)
        _assert_windows_refilled(name, opt, n, stats)
        if opt == "default":
            tm = wc.templates(n)
            at0 = [O.evaluate(fm, O.transform(tm[r["tmpl_idx"]], r["transform"]), [(0.0, 0.0)])[0] for r in rec]
            wc.same_bits(at0, rec["score"], f"{name} {n} lines: the score at translation 0")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("name", ["valley61", "valley61-t"])
def test_valley_stops_inside_the_range(backend, opt, name):
    """The valley's minimum lies strictly inside the range: no record at the far edge, none at the alignment."""
    plateau = "plateau-t" if wc.transposed(name) else "plateau"
    for n in wc.LINE_COUNTS:
        rec, _ = _search(backend, name, opt, n)
        assert (wc.moved_max(name, rec, n) < wc.SIZE - 2).all(), (name, opt, n)
        assert (wc.multipliers(name, rec, wc.oracle_search(plateau, "default", n)[0]) > 0).all(), (name, opt, n)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("opt", SMALL)
@pytest.mark.parametrize("suffix", ["", "-t"], ids=["x", "y"])
def test_valley_sweep_stops_at_every_residue(backend, opt, suffix):
    """Witness 4: as the valley moves over 16 consecutive pixels the best multipliers take every residue modulo B (for
    B = 1 modulo 15, the window): the walk stops at every position of a batch and of a window."""
    B = wc.OPTIMISERS[opt][1]
    ks = []
    for c in wc.SWEEP:
        name = f"valley{c}{suffix}"
        for n in SWEEP_COUNTS:
            rec, _ = _search(backend, name, opt, n)
            ks.append(wc.multipliers(name, rec, wc.oracle_search("plateau" + suffix, "default", n)[0]))
    ks = np.abs(np.concatenate(ks))
    assert set(ks % B) == set(range(B)), (opt, sorted(set(ks % B)))
    if B == 1:
        assert set(ks % 15) == set(range(15)), sorted(set(ks % 15))


@pytest.mark.parametrize("name", wc.VOLUMES)
def test_indulgent_scores_a_rejected_translation_again(name):
    """IndulgentOptimize(p) scores a translation it rejects p more times before it gives up, and walks exactly like
    IndulgentOptimize(0): same records, p more scorings per direction that ends in a rejection.  fdcm_search_timing
    counts translations, each once (walk_cases.device_evaluations; asserted on the device by every case above).  On the
    ramp exactly one direction of every candidate ends in a rejection, on the plateau none."""
    for n in wc.LINE_COUNTS:
        rec3, st3 = wc.oracle_search(name, "indulgent3", n)
        rec0, st0 = wc.oracle_search(name, (O.INDULGENT_OPTIMIZE, 0), n)
        wc.same_records(rec3, rec0, f"{name} {n} lines")
        again, cands = wc.evaluations(st3, n) - wc.evaluations(st0, n), int(st3[1])
        assert again % 3 == 0 and 0 <= again <= 2 * 3 * cands, (name, n, again, cands)
        if name.startswith("ramp"):
            assert again == 3 * cands, (name, n, again, cands)
        if name.startswith("plateau"):
            assert again == 0, (name, n, again)


# ------------------------------------------------------------------------------------------------ LDS (device only)
@pytest.mark.gpu
def test_lds_above_64k_through_lines():
    """One template of 900 lines, B = 1: 72 560 bytes of dynamic LDS, more than a kernel gets without asking."""
    assert wc.lds_bytes(900, 1) == 72560 > 64 * 1024
    assert len(wc.templates(900)) == 1
    wc.check_device("valley61", "default", 900)


@pytest.mark.gpu
def test_lds_above_64k_through_batch():
    """BatchOptimize(4096) with templates of 9 lines: two score windows of 4096, about 132 KB."""
    assert 128 * 1024 < wc.lds_bytes(9, 4096) <= 160 * 1024
    wc.check_device("ramp", "batch4096", 9)


@pytest.mark.gpu
def test_lds_refusal_leaves_the_handle_usable():
    """A template of 2042 lines needs 163 920 bytes, more than the 160 KB a workgroup has: refused before any GPU work, and
    the next search on the same handle is the oracle's."""
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import search_raw
    assert wc.lds_bytes(2042, 1) == 163920 > 160 * 1024 >= wc.lds_bytes(2041, 1)
    dev = wc.device_map("valley61")
    for _ in range(2):
        with pytest.raises(_capi.FdcmError, match="LDS staging"):
            search_raw(dev, wc.device_templates(2042), wc.scene(False), 4, 4, O.DEFAULT_OPTIMIZE, 1)
        wc.check_device("valley61", "batch7", 9)


# ------------------------------------------------------------------------------------------------ both address forms
@pytest.mark.gpu
def test_walks_with_64_bit_addresses():
    """Every volume, optimiser and line count once more with FDCM_SEARCH_FLAT=1 (the form volumes of 4 GB and more take),
    in a process of its own: the switch is read once.  There a read past the last admissible multiplier is a read outside
    the slice, not a zero."""
    import os
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "walk_cases.py")
    out = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300,
                         env={**os.environ, "FDCM_SEARCH_FLAT": "1"})
    want = len(wc.VOLUMES) * len(wc.OPTIMISERS) * len(wc.LINE_COUNTS)
    assert out.returncode == 0 and f"{want} walk searches identical" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
