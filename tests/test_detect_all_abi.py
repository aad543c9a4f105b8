"""Checks of "all detections below a score" (include/fdcm.h) that need no scene: the library exports the entry points and
the binding knows them; every argument check returns FDCM_EINVAL with a message before any handle or device is touched; the
bound of a denominator by definition; the referee's bisection against the library's; and the arithmetic of the early exit's
proof on random term vectors.  One test needs template handles, which need a device: it is marked."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from capped_ref import eigen_sum0
from detect_all_ref import EXIT_MAX_LINES, denominators, exit_bound, exit_checks, score_bound

EINVAL = -1
f32 = np.float32
INF = f32(np.inf)
NEW_SYMBOLS = ["fdcm_search_exhaustive_detect_all", "fdcm_detect_score_bounds", "fdcm_score_bound"]
SUBNORMAL = np.array([1], dtype=np.uint32).view(np.float32)[0]
MAX_SCORES = [f32(0), SUBNORMAL, f32(0.3), f32(1), f32(2.5), f32(1e30), INF]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _all(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), max_score=1.0, max_det=8, permille=300, margin=0, penalty=-1, tau=1.0, out=True,
         n_out=True, boxes=False):
    o, n = C.c_void_p(), C.c_int64()
    b = np.zeros(4 * 4096, dtype=np.int32)
    g = capi.Grid(*grid) if grid is not None else None
    return capi.lib().fdcm_search_exhaustive_detect_all(
        None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None, max_score, max_det, permille,
        margin, penalty, tau, 0, C.byref(o) if out else None, C.byref(n) if n_out else None,
        b.ctypes.data_as(C.POINTER(C.c_int32)) if boxes else None)


def _bound(capi, den, max_score):
    out = C.c_float()
    assert capi.lib().fdcm_score_bound(float(den), float(max_score), C.byref(out)) == 0
    return f32(out.value)


def test_exports_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    assert len(bound["fdcm_search_exhaustive_detect_all"][2]) == 14 and bound["fdcm_search_exhaustive_detect_all"][2][4] is C.c_float
    assert len(bound["fdcm_detect_score_bounds"][2]) == 5
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    p = inspect.signature(fd.exhaustive_detect_all).parameters
    assert list(p)[:3] == ["featuremap", "templates", "max_score"] and p["max_score"].default is inspect.Parameter.empty
    assert p["overlap"].default == 0.3 and p["stride"].default == 1 and p["max_detections"].default == 1024
    assert p["penalty"].default is None and p["angles"].default is None and p["pivot"].default == "center"
    assert p["window"].default is None and p["line_caps"].default is None and p["margin"].default == 0
    assert p["return_boxes"].default is False
    p = inspect.signature(DeviceFeatureMap.exhaustive_detect_all).parameters
    assert p["max_detections"].default == 1024 and p["overlap_permille"].default == 300 and p["margin"].default == 0
    assert p["penalty"].default is None and p["tau"].default == 1.0 and p["tmpl_index_base"].default == 0 and p["boxes"].default is False
    assert list(inspect.signature(fd.detect_score_bounds).parameters) == ["templates", "penalty", "max_score"]
    assert callable(DeviceTemplates.score_bounds)
    # the calls that were there keep their signatures
    p = inspect.signature(fd.exhaustive_detect_nms).parameters
    assert p["k"].default == 8 and "max_score" not in p
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in header


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the call goes on to the (null) handles."""
    for ms, md in [(0.0, 1), (-0.0, 4096), (np.inf, 64), (float(SUBNORMAL), 65), (2.5, 1024)]:
        assert _all(capi, max_score=ms, max_det=md, boxes=True) == EINVAL
        assert "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("max_score", [np.nan, -1.0, -np.inf, -1e-30, -float(SUBNORMAL)])
def test_bad_max_score_is_einval(capi, max_score):
    assert _all(capi, max_score=max_score) == EINVAL and "max_score must be >= 0" in _err(capi)
    out = C.c_float()
    assert capi.lib().fdcm_score_bound(1.0, max_score, C.byref(out)) == EINVAL and "max_score must be >= 0" in _err(capi)
    b = np.zeros(4, dtype=np.float32)
    assert capi.lib().fdcm_detect_score_bounds(None, -1, 1.0, max_score, capi.fptr(b)) == EINVAL
    assert "max_score must be >= 0" in _err(capi)


@pytest.mark.parametrize("max_det", [0, 4097, -1, 1 << 30])
def test_max_detections_out_of_range_is_einval(capi, max_det):
    assert _all(capi, max_det=max_det) == EINVAL and "max_detections must be in [1, 4096]" in _err(capi)


def test_what_the_nms_call_rejects_is_einval(capi):
    for permille in (-1, 1001):
        assert _all(capi, permille=permille) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)
    for margin in (-1, 4097):
        assert _all(capi, margin=margin) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert _all(capi, out=False) == EINVAL and "null output" in _err(capi)
    assert _all(capi, n_out=False) == EINVAL and "null output" in _err(capi)
    assert _all(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    for grid, what in [((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26")]:
        assert _all(capi, grid=grid) == EINVAL and what in _err(capi)
    for penalty in (-2, 2):
        assert _all(capi, penalty=penalty) == EINVAL and "unknown penalty" in _err(capi)
    for tau in (np.nan, np.inf):
        assert _all(capi, penalty=1, tau=tau) == EINVAL and "tau must be finite" in _err(capi)
    cs = np.float32([[1, 0], [np.nan, 0]])
    r = capi.Rotations(capi.fptr(cs), 2, None)
    assert _all(capi, rot=r) == EINVAL and "c and s must be finite" in _err(capi)
    assert _all(capi, rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)
    assert _all(capi) == EINVAL and "null featuremap/templates" in _err(capi)  # rot and boxes_out may be null, the handles not
    b = np.zeros(4, dtype=np.float32)
    f = capi.lib().fdcm_detect_score_bounds
    assert f(None, -1, 1.0, 1.0, capi.fptr(b)) == EINVAL and "templates is null" in _err(capi)
    assert f(None, 5, 1.0, 1.0, capi.fptr(b)) == EINVAL and "unknown penalty" in _err(capi)
    assert f(None, 1, np.nan, 1.0, capi.fptr(b)) == EINVAL and "tau must be finite" in _err(capi)
    assert capi.lib().fdcm_score_bound(1.0, 1.0, None) == EINVAL and "bound is null" in _err(capi)


def _by_definition(B, den, max_score):
    """B is the largest s >= +0 with float32(s / den) <= max_score."""
    with np.errstate(all="ignore"):
        assert B >= 0 and f32(B / f32(den)) <= max_score
        if B != INF:
            assert f32(np.nextafter(f32(B), INF) / f32(den)) > max_score


def test_score_bound_by_definition(capi):
    """fdcm_score_bound over denominators of every size (lengths and their powers lie in 1e-6 .. 1e12), against the
    definition and against the referee's own bisection."""
    rng = np.random.default_rng(5)
    dens = np.concatenate([f32([1e-6, 1, 3, 0.1, 7.3, 1e6, 1e12, 2.0 ** -126, 2.0 ** 100]),
                           np.exp(rng.uniform(np.log(1e-6), np.log(1e12), 300)).astype(np.float32)])
    hit_inf = hit_zero = 0
    for ms in MAX_SCORES:
        for den in dens:
            B = _bound(capi, den, ms)
            _by_definition(B, den, ms)
            assert B.tobytes() == f32(score_bound(den, ms)).tobytes()
            hit_inf += B == INF
            hit_zero += B == 0
    assert hit_inf >= len(dens) and hit_zero > 0  # +inf at max_score = +inf; 0 where even the smallest subnormal is over
    assert _bound(capi, 1.0, 0.3) == f32(0.3) and _bound(capi, 1.0, np.inf) == INF and _bound(capi, 1.0, 0.0) == 0
    # denominators no template has: the ends of the definition
    assert _bound(capi, np.inf, 1.0) == np.finfo(np.float32).max and _bound(capi, 0.0, np.inf) == INF and _bound(capi, 0.0, 5.0) == 0


@pytest.mark.gpu
def test_detect_score_bounds_by_definition():
    """fdcm_detect_score_bounds on ragged sets (a handle needs a device), each penalty, tau in {1, 1.5}: per template B with
    float32(B / den) <= max_score < float32(nextafter(B) / den).  The quotient is taken as the header defines q, by
    fdcm_penalize on the handle's lengths, and for the penalties whose den is exact in numpy (none, the default one, and
    tau = 1, where the power is the length itself) also with den recomputed from fdcm_templates_lengths."""
    from detect_ref import normalised
    from openfdcm_amd.engine import DeviceTemplates
    rng = np.random.default_rng(11)
    sets = []
    for sizes in ([0, 1, 3, 40], [5, 0, 0, 17, 2, 33, 8], [1]):
        sets.append([rng.uniform(-60, 60, (4, n)).astype(np.float32) * f32(10.0 ** rng.integers(-3, 3)) for n in sizes])
    sets[1][2] = np.zeros((4, 0), dtype=np.float32)
    sets[0][1] = np.zeros((4, 1), dtype=np.float32)  # a line of length 0: den = 1e-6
    for tmpls in sets:
        tset = DeviceTemplates(tmpls)
        lens = tset.lengths()
        empty = np.array([t.shape[1] == 0 for t in tmpls])
        for penalty, tau in [(None, 1.0), (0, 1.0), (1, 1.0), (1, 1.5)]:
            for ms in MAX_SCORES:
                B = tset.score_bounds(ms, penalty=penalty, tau=tau)
                assert B.dtype == np.float32 and B.shape == (len(tmpls),) and np.all(B[empty] == 0)
                up = np.where(B == INF, INF, np.nextafter(B, INF))
                q = normalised(np.stack([B, up], axis=1)[:, :, None, None], lens, penalty, tau)[:, :, 0, 0]
                live = ~empty
                assert np.all(q[live, 0] <= ms) and np.all((q[live, 1] > ms) | (B[live] == INF))
                if (penalty, tau) != (1, 1.5):
                    for t in np.flatnonzero(live):
                        _by_definition(B[t], denominators(lens, penalty, tau)[t], ms)
    assert DeviceTemplates([]).score_bounds(1.0).shape == (0,)


def test_exit_bound_is_the_documented_factor():
    """Bc >= B / (1 - 2 n u) exactly (in rationals), and it is within 3 float32 steps of it; off for B = inf and n > 2^20."""
    from fractions import Fraction
    u = Fraction(1, 1 << 24)
    for B in [f32(0), SUBNORMAL, f32(0.3), f32(17.25), f32(1e-20), f32(1e30), f32(8e37)]:
        for n in (1, 8, 33, 70, 1000, EXIT_MAX_LINES):
            c = exit_bound(B, n)
            assert c != INF and Fraction(float(c)) * (1 - 2 * n * u) >= Fraction(float(B))
            lo = c
            for _ in range(3):
                lo = np.nextafter(lo, f32(-1))
            assert lo < 0 or Fraction(float(lo)) * (1 - 2 * n * u) < Fraction(float(B)) or B == 0
    assert exit_bound(INF, 5) == INF and exit_bound(f32(1.0), EXIT_MAX_LINES + 1) == INF and exit_bound(f32(2e38), 8) == INF


def test_exit_rule_is_one_sided():
    """The rule the kernel uses -- abandon a slot when C > Bc, C the float32 sum of its accumulators at a check, Bc =
    exit_bound(B, n) -- never drops a point the full sum would keep: on 20 000 random term vectors (n in 1 .. 70, magnitudes
    1e-30 .. 1e30, zeros, inf and NaN among them), summed in the order of capped_ref's Eigen sum, "dropped at some check"
    implies "final > B or NaN".  B is drawn near the partial sums and the final sum, where the rule is tight."""
    rng = np.random.default_rng(2024)
    dropped = kept = specials = 0
    for it in range(20000):
        n = int(rng.integers(1, 71))
        span = rng.choice([0.5, 3, 30])
        shift = rng.uniform(-30, 30) if it % 3 == 0 else 0.0
        v = (10.0 ** np.clip(shift + rng.uniform(-span, span, n), -30, 30)).astype(np.float32)
        if it % 4 == 0:
            v[rng.random(n) < 0.3] = 0
        if it % 50 == 1:
            v[rng.integers(0, n)] = np.inf
        if it % 50 == 2:
            v[rng.integers(0, n)] = np.nan
        if it % 50 == 3:
            v[:] = rng.choice([1e30, 3e37, 1e38])  # sums that overflow
        final = eigen_sum0(v)
        checks = exit_checks(v)
        assert len(checks) == n // 8 - (n >= 8 and n % 8 == 0) + (n % 8 > 4)  # a check only where lines remain
        anchors = [final] + [c for c in checks if np.isfinite(c)]
        for _ in range(3):
            a = f32(anchors[int(rng.integers(0, len(anchors)))])
            B = f32(a * f32(1 - rng.choice([0, 1, 2, 4]) * n * 2.0 ** -24)) if np.isfinite(a) else f32(1.0)
            for _ in range(int(rng.integers(0, 4))):
                B = np.nextafter(B, f32(rng.choice([-1, 1]) * np.inf))
            B = f32(abs(B)) if np.isfinite(B) else f32(1.0)
            Bc = exit_bound(B, n)
            with np.errstate(invalid="ignore"):
                drop = any(c > Bc for c in checks)
            if drop:
                dropped += 1
                assert np.isnan(final) or final > B, (n, B, Bc, final, checks)
            else:
                kept += 1
        specials += not np.isfinite(final)
    print("dropped", dropped, "kept", kept, "vectors with a final that is not finite", specials)
    assert dropped > 5000 and kept > 5000 and specials > 300
