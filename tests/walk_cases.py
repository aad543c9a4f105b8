"""Designed volumes that walk the line-search optimiser to the map's edge, and the witnesses that it got there.

On a DT3 volume built from a scene a descent ends after a batch or two, so a comparison with the oracle never reaches the
windows the kernel scores after its first one, the last admissible multiplier of minmaxTranslation, a walk through equal
scores, or a batch that is split into pieces.  Adopted volumes (O.from_volume, DeviceFeatureMap.from_volume) take any
integrated volume, so here the volume is a function of x alone (or, transposed, of y alone) in m = 4 equal slices -- the
orientation bins do not matter -- and the scene lines are nearly parallel to that axis: the scaled align vector has
abs(sav.x) == 1 (abs(sav.y) == 1), every multiplier moves the template by one whole pixel along the axis, and a walk is
about 100 multipliers long.

  ramp       I = 2^-x     |2^-(x1 + k) - 2^-(x2 + k)| = 2^-k |2^-x1 - 2^-x2| exactly (2^-111 is a normal float32): the
                          score falls strictly towards +x, the rule walks to the last admissible multiplier
  plateau    I = 3 x      |3 (x1 + k) - 3 (x2 + k)| does not depend on k: every multiplier scores the same bits, the rule
                          walks the whole range in both directions and the first minimum (multiplier 0) wins
  valley(c)  I = (x - c)^2   a sum of V shapes |x1 - x2| |x1 + x2 + 2 k - 2 c| in integers below 2^24: convex, the minimum
                          strictly inside the range, one pixel further for c + 1

The witnesses are computed from the oracle's records and statistics alone, so they hold (or fail) without a GPU.  The
properties above are exact as long as no moved end point comes within a float32 rounding of a pixel edge (the sum
coordinate + translation is rounded at another magnitude for every multiplier); should a change of the generators put
one there, the plateau witness fails on the oracle: take another seed, the bounds stay.

Reads stay inside the slice at the last multiplier: minmaxTranslation bounds k by (size - 1 - max) / sav with abs(sav) = 1
along the walk, so max + k <= size - 1 up to a few float32 roundings of values below 128, and the truncated pixel index is
at most size - 1; at the low end min + k >= 0 up to the same roundings, and anything in (-1, 0) truncates to pixel 0.
"""
import functools

import numpy as np

from helpers import definition_keys
from oracle import oracle as O

M = 4
SIZE, ACROSS = 112, 40                  # along the walk, across it
T_ALONG, T_ACROSS = -2.75, 0.125        # the scene translation
LINE_COUNTS = (1, 3, 4, 8, 9, 33, 64, 65, 130)
PER_COUNT = 5                           # templates of every line count: 160 candidates from 4 lines on
BATCHES = (1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 1000, 4096)
OPTIMISERS = {"default": (O.DEFAULT_OPTIMIZE, 1), "indulgent3": (O.INDULGENT_OPTIMIZE, 3),
              **{f"batch{B}": (O.BATCH_OPTIMIZE, B) for B in BATCHES}}
SWEEP = tuple(range(46, 62))            # valley(c): 16 consecutive minima
VOLUMES = ("ramp", "plateau", "valley61", "ramp-t", "plateau-t", "valley61-t")


def window(B):
    """Multipliers the kernel scores per direction and round (run_search)."""
    return (15 // B) * B if B <= 15 else B


def lds_bytes(max_lines, B, m=M):
    """Dynamic LDS of the search kernel: four waves of keys | 5 floats per line | two windows and the zero slot."""
    return 16 * (m + 5 * max_lines + 2 * window(B) + 1)


def transposed(name):
    return name.endswith("-t")


@functools.lru_cache(maxsize=None)
def volume(name):
    """(volume (m, W, H) float32 [k][x][y], keys, scene translation) of 'ramp', 'plateau', 'valley<c>' or their
    transposes ('-t': a function of y, 40 x 112).  Every value is exact in float32."""
    base = name[:-2] if transposed(name) else name
    x = np.arange(SIZE, dtype=np.float64)
    col = {"ramp": 2.0 ** -x, "plateau": 3.0 * x}.get(base)
    if col is None:
        assert base.startswith("valley"), name
        col = (x - int(base[len("valley"):])) ** 2
    col32 = col.astype(np.float32)
    assert np.array_equal(col32.astype(np.float64), col) and (col32[col != 0] >= np.finfo(np.float32).tiny).all()
    if transposed(name):
        vol = np.broadcast_to(col32[None, None, :], (M, ACROSS, SIZE))
        T = np.array([T_ACROSS, T_ALONG], dtype=np.float32)
    else:
        vol = np.broadcast_to(col32[None, :, None], (M, SIZE, ACROSS))
        T = np.array([T_ALONG, T_ACROSS], dtype=np.float32)
    vol = np.ascontiguousarray(vol)
    vol.setflags(write=False)
    return vol, definition_keys(M).astype(np.float32), T


@functools.lru_cache(maxsize=None)
def scene(is_transposed):
    """(4, 6) float32 scene lines in scene coordinates: length 4 to 9, slope within 0.04 of the axis, every second one
    reversed (sav = +1 and -1 along the axis), the low end at 8..30 along and 14..26 across."""
    rng = np.random.default_rng(20261019)
    n = 6
    a0, c0 = rng.uniform(8, 30, n), rng.uniform(14, 26, n)
    length, slope = rng.uniform(4, 9, n), rng.uniform(-0.04, 0.04, n)
    a1 = a0 + length / np.sqrt(1 + slope ** 2)
    c1 = c0 + slope * (a1 - a0)
    s = np.stack([a0, c0, a1, c1])
    s[:, 1::2] = s[[2, 3, 0, 1]][:, 1::2]
    s = s[[1, 0, 3, 2]] if is_transposed else s
    s = np.ascontiguousarray(s, dtype=np.float32)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def templates(n, seed=0):
    """PER_COUNT templates of n random lines (one template above 130 lines: the LDS cases) within 2.4 of the origin on
    either axis (every aligned copy stays inside the map across the walk), no line shorter than 1.5 pixels: the end points
    of the line that lies along the scene line fall into different pixels along the walk, so a template of one line does
    not score 0 everywhere."""
    rng = np.random.default_rng(1000 * seed + n)
    out = []
    for _ in range(PER_COUNT if n <= 130 else 1):
        t = rng.uniform(-2.4, 2.4, size=(4, n))
        while True:
            short = np.hypot(t[2] - t[0], t[3] - t[1]) < 1.5
            if not short.any():
                break
            t[:, short] = rng.uniform(-2.4, 2.4, size=(4, int(short.sum())))
        t = t.astype(np.float32)
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_map(name):
    vol, keys, T = volume(name)
    return O.from_volume(keys, vol, T)


@functools.lru_cache(maxsize=None)
def oracle_search(name, opt, n, seed=0):
    """(records, stats) of DefaultSearch(4, 4) with OPTIMISERS[opt] (or a (kind, batch) pair) on the volume, for the
    templates of n lines.  Computed once and shared: read-only."""
    kind, batch = OPTIMISERS[opt] if isinstance(opt, str) else opt
    rec, stats = O.search(oracle_map(name), list(templates(n, seed)), scene(transposed(name)), 4, 4, kind=kind, batch=batch,
                          nthreads=4, return_stats=True)
    rec.setflags(write=False)
    stats.setflags(write=False)
    return rec, stats


def evaluations(stats, n):
    """Scorings of a translation by the reference rule: the oracle counts two volume reads per line and scoring."""
    reads, per = int(stats[0]), 2 * n
    assert reads % per == 0, (reads, n)
    return reads // per


def device_evaluations(name, opt, n, seed=0):
    """What fdcm_search_timing.evaluations holds after the same search (include/fdcm.h): the translations the rule scores,
    each once.  DefaultOptimize and BatchOptimize score no translation twice; IndulgentOptimize scores a rejected one
    again once per allowed pass-through, so its count is the rule's with no pass-through allowed."""
    kind, batch = OPTIMISERS[opt] if isinstance(opt, str) else opt
    if kind == O.INDULGENT_OPTIMIZE:
        return evaluations(oracle_search(name, (kind, 0), n, seed)[1], n)
    return evaluations(oracle_search(name, opt, n, seed)[1], n)


def moved_max(name, rec, n, seed=0):
    """Per record the largest coordinate along the walk of the template moved by the record's transform and the scene
    translation (float64 from the float32 values)."""
    T = volume(name)[2].astype(np.float64)
    r = 1 if transposed(name) else 0
    tm = templates(n, seed)
    out = np.zeros(len(rec))
    for i, q in enumerate(rec):
        A = q["transform"].astype(np.float64).reshape(2, 3)
        pts = tm[q["tmpl_idx"]].astype(np.float64).reshape(2, -1, order="F")
        out[i] = (A[r, :2] @ pts + A[r, 2] + T[r]).max()
    return out


def multipliers(name, rec, rec_plateau):
    """The best multiplier of every record as a distance in pixels: the record's translation along the walk minus that of
    the plateau record at the same position (multiplier 0: the alignment itself).  abs(sav) == 1 along the walk."""
    assert len(rec) == len(rec_plateau) and np.array_equal(rec["tmpl_idx"], rec_plateau["tmpl_idx"])
    c = 5 if transposed(name) else 2
    d = rec["transform"][:, c].astype(np.float64) - rec_plateau["transform"][:, c].astype(np.float64)
    k = np.rint(d)
    assert np.abs(d - k).max(initial=0) < 1e-3, np.abs(d - k).max()
    return k.astype(np.int64)


def same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {idx}: got {got[idx]!r} want {want[idx]!r}")


def same_records(got, want, what):
    """Positionally the same records, byte for byte (NaN equal to NaN)."""
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"]), what
    same_bits(got["score"], want["score"], what + " score")
    same_bits(got["transform"], want["transform"], what + " transform")


# ------------------------------------------------------------------------------------------------ the device side
_device_maps, _device_templates = {}, {}


def device_map(name):
    """One handle per volume, kept for every optimiser and line count."""
    if name not in _device_maps:
        from openfdcm_amd.engine import DeviceFeatureMap
        vol, keys, T = volume(name)
        _device_maps[name] = DeviceFeatureMap.from_volume(keys, vol, T)
    return _device_maps[name]


def device_templates(n, seed=0):
    if (n, seed) not in _device_templates:
        from openfdcm_amd.engine import DeviceTemplates
        _device_templates[n, seed] = DeviceTemplates(list(templates(n, seed)))
    return _device_templates[n, seed]


def device_search(name, opt, n, seed=0):
    """(records, evaluations, candidates) of the library for the search of oracle_search."""
    from openfdcm_amd.engine import search_raw
    kind, batch = OPTIMISERS[opt] if isinstance(opt, str) else opt
    dev = device_map(name)
    rec = search_raw(dev, device_templates(n, seed), scene(transposed(name)), 4, 4, kind, batch)
    st = dev.search_timing()
    return rec, st["evaluations"], st["candidates"]


def check_device(name, opt, n, seed=0):
    """The library's records are the oracle's, its candidate and evaluation counts the rule's."""
    want, stats = oracle_search(name, opt, n, seed)
    got, evals, cands = device_search(name, opt, n, seed)
    what = f"{name} {opt} {n} lines"
    same_records(got, want, what)
    assert cands == stats[1], (what, cands, int(stats[1]))
    assert evals == device_evaluations(name, opt, n, seed), (what, evals, device_evaluations(name, opt, n, seed))


if __name__ == "__main__":   # every volume, optimiser and line count on the device, in a process of its own
    done = 0
    for name_ in VOLUMES:
        for opt_ in OPTIMISERS:
            for n_ in LINE_COUNTS:
                check_device(name_, opt_, n_)
                done += 1
    print(f"{done} walk searches identical")
