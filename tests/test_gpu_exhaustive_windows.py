"""GPU tests of the pose-window search (include/fdcm.h, "Pose windows").  The volumes the records are judged by are the
oracle's evaluate on host-rotated lines at every admissible point of a stride-1 master grid, admissibility by the header's
rule in numpy (windows_ref.py): nothing of the device's own maps.  Then the identity, job by job, against
fdcm_search_exhaustive_rotations on the one-template set (the one cross-check against existing device code), adopted
volumes (all zero: ties; a NaN and an infinity), translations only against fdcm_search_exhaustive, the test switches in
fresh processes, the public Python surface and the argument checks that need a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from rotation_ref import rotate_lines, rotated_set
from test_gpu_exhaustive import _grid_points, _templates_with_sizes
from windows_ref import admissible_mask, window_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASTER = (-200, -190, 264, 262)  # stride 1; the map is 307 x 307 with scene translation 25.5: admissible x begin near -125
DEG = [0, 20, 45, 90, 135, 180, 250, 330]
N = len(DEG)
WINDOWS = [(1, 1), (3, 3), (5, 2), (17, 65), (64, 16)]
RUNS = [(0, 1), (0, N), (6, 4), (3, 1), (2, 5), (7, 1), (7, 3)]  # (6, 4) and (7, 3) cross n - 1 -> 0
LINES = [0, 5, 12, 23, 8, 9, 16, 3]  # lines per template of the fixture
WITH_LINES = range(1, len(LINES))


def _cs(deg):
    a = np.deg2rad(np.asarray(deg, dtype=np.float64))
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


CS = _cs(DEG)


def _centers(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, tm in enumerate(tmpls):
        if tm.shape[1]:
            xs, ys = np.concatenate([tm[0], tm[2]]), np.concatenate([tm[1], tm[3]])
            out[t] = [(xs.min() + xs.max()) / np.float32(2), (ys.min() + ys.max()) / np.float32(2)]
    return out


def _oracle_volume(orc, sets, master):
    """(len(sets), NY, NX): the oracle's evaluate of each line set at every admissible point of the master grid."""
    X0, Y0, NX, NY = master
    pts = _grid_points((X0, Y0, NX, NY, 1, 1)).reshape(-1, 2)
    vol = np.full((len(sets), NY * NX), np.nan, dtype=np.float32)
    for a, lines in enumerate(sets):
        adm = admissible_mask(lines, orc.translation, orc.W, orc.H, master).reshape(-1)
        vol[a, adm] = O.evaluate(orc, lines, pts[adm])
    return vol.reshape(len(sets), NY, NX)


@pytest.fixture(scope="module")
def world():
    """A 307 x 307 x 12 map and templates of every shape of the sum (rows_score): no lines; 5 = the packet and one tail
    line; 12 = a block of 8 and the packet; 23 = two blocks, the packet and a tail of 3; 8 and 16 = blocks alone; 9 = a block
    and a tail without a packet; 3 = the tail alone.  Per template with lines its oracle volumes over the 8 rotations and
    over the lines as they are.  Computed once and left unchanged."""
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene = synthetic.scene(256, 48, 9)
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.2, distance=0)
    orc = O.build(scene, depth=12, coeff=5.0, padding=1.2, distance=O.L2, nthreads=8)
    assert (dev.width, dev.height) == (orc.W, orc.H) and np.array_equal(dev.scene_translation, orc.translation)
    rng = np.random.default_rng(31)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, LINES)
    piv = _centers(tmpls)
    rs = rotated_set(tmpls, CS, piv)
    vols = [None] + [_oracle_volume(orc, rs[t * N:(t + 1) * N], MASTER) for t in WITH_LINES]
    vols0 = [None] + [_oracle_volume(orc, [tmpls[t]], MASTER) for t in WITH_LINES]
    for v in vols[1:]:
        v.setflags(write=False)
        assert (~np.isnan(v)).sum() > 100000
    return dict(dev=dev, orc=orc, tmpls=tmpls, tset=DeviceTemplates(tmpls), piv=piv, vols=vols, vols0=vols0)


def _place(x, n, s, lo, hi):
    """x, moved down until the window's last point is inside [lo, hi]."""
    return max(lo, min(x, hi - (n - 1) * s))


def _jobs(sx, sy, wrap):
    """Every window shape at four places -- inside the admissible boxes, across their left edge, left of them (nothing
    admissible) and across their upper edge -- with x0 at each residue mod 4, for every template with lines, the runs
    taken in turn."""
    X1, Y1 = MASTER[0] + MASTER[2] - 1, MASTER[1] + MASTER[3] - 1
    jobs, q = [], 0
    for t in WITH_LINES:
        for nx, ny in WINDOWS:
            for xa, ya in [(-60, -50), (-132, -60), (-199, -40), (-70, -175)]:
                for r in range(4):
                    a0, na = RUNS[q % len(RUNS)]
                    q += 1
                    if not wrap and a0 + na > N:
                        a0, na = N - 1, 1
                    jobs.append((t, a0, na, _place(xa + r, nx, sx, MASTER[0], X1), _place(ya, ny, sy, MASTER[1], Y1), nx, ny))
    return np.asarray(jobs, dtype=np.int32)


def _same(got, want):
    (rec, off), (wrec, woff) = got, want
    assert np.array_equal(off, woff)
    assert np.array_equal(rec["tmpl_idx"], wrec["tmpl_idx"])
    assert rec["score"].tobytes() == wrec["score"].tobytes()
    assert rec["transform"].tobytes() == wrec["transform"].tobytes()


@pytest.mark.parametrize("stride", [(1, 1), (2, 2), (3, 3), (4, 2)])
def test_against_the_referee_on_the_oracle_volumes(world, stride):
    sx, sy = stride
    dev, tset, piv, vols = world["dev"], world["tset"], world["piv"], world["vols"]
    for wrap in ((True, False) if stride == (1, 1) else (True,)):
        jobs = _jobs(sx, sy, wrap)
        assert len({int(j[3]) % 4 for j in jobs}) == 4
        for k in (1, 8, 64):
            got = dev.exhaustive_window_search(tset, jobs, CS, piv, sx=sx, sy=sy, wrap=wrap, k=k, tmpl_index_base=5)
            _same(got, window_records(vols, MASTER, jobs, CS, piv, k, sx, sy, wrap, base=5))
        cnt = np.diff(got[1])
        pts = jobs[:, 2] * jobs[:, 5] * jobs[:, 6]
        full = cnt == np.minimum(64, pts)
        assert (cnt == 0).sum() >= 20 and full.sum() >= 20 and ((cnt > 0) & ~full).sum() >= 5  # outside, inside, across
        assert ((cnt < 64) & (cnt > 0)).any()  # count < k


def _patches(vols, jobs):
    """The 4 x 16 patches of a stride-1 job list: per (job, run position) the bounding box of the window's admissible points
    (the admissible set is a box), read off the volumes."""
    n = 0
    for t, a0, na, x0, y0, nx, ny in jobs:
        for e in range(na):
            adm = ~np.isnan(vols[t][(a0 + e) % N][y0 - MASTER[1]:y0 - MASTER[1] + ny, x0 - MASTER[0]:x0 - MASTER[0] + nx])
            if adm.any():
                jj, ii = np.nonzero(adm)
                n += ((ii.max() - ii.min()) // 4 + 1) * ((jj.max() - jj.min()) // 16 + 1)
    return int(n)


def test_many_patches_per_wave_and_jobs_that_share_a_wave(world):
    """One batch of more than 4 x 16 384 patches, so a wave takes 5 or more (ipw = ceil(patches / 16 384)): large jobs of
    8 x 128 x 64 and 256 x 140 points between small ones of odd sizes, whose patch counts are no multiple of any ipw.  Job
    boundaries fall inside waves -- a wave writes one list per job it holds patches of and starts the next from empty --
    and whole small jobs lie inside one wave.  Judged by the referee on the oracle's volumes; the same list reversed
    (other waves, other boundaries) gives the same records per job."""
    dev, tset, piv, vols = world["dev"], world["tset"], world["piv"], world["vols"]
    rng = np.random.default_rng(17)
    small = [(1, 1), (3, 3), (5, 2), (17, 65), (9, 9), (6, 19), (64, 16)]
    jobs, patches = [], 0
    for q in range(100):
        t = 1 + q % (len(LINES) - 1)
        if q % 2:
            jobs.append((t, 0, N, int(rng.integers(-130, -70)), int(rng.integers(-70, -50)), 128, 64))
        else:
            jobs.append((t, int(rng.integers(0, N)), 1, int(rng.integers(-199, -192)), int(rng.integers(-80, -70)), 256, 140))
        for _ in range(int(rng.integers(1, 5))):
            nx, ny = small[int(rng.integers(0, len(small)))]
            a0, na = RUNS[int(rng.integers(0, len(RUNS)))]
            jobs.append((1 + int(rng.integers(0, len(LINES) - 1)), a0, na, int(rng.integers(-140, -20)), int(rng.integers(-120, -10)), nx, ny))
    jobs = np.asarray(jobs, dtype=np.int32)
    assert np.all(jobs[:, 2] * jobs[:, 5] * jobs[:, 6] <= 65536) and jobs[:, 2].sum() < 65536
    for k in (1, 64):
        got = dev.exhaustive_window_search(tset, jobs, CS, piv, wrap=True, k=k)
        _same(got, window_records(vols, MASTER, jobs, CS, piv, k, 1, 1, True))
    assert _patches(vols, jobs) > 4 * 16384
    rec, off = got
    back = dev.exhaustive_window_search(tset, jobs[::-1], CS, piv, wrap=True, k=64)
    for j in range(len(jobs)):
        r = len(jobs) - 1 - j
        assert rec[off[j]:off[j + 1]].tobytes() == back[0][back[1][r]:back[1][r + 1]].tobytes(), j


def test_limit_jobs_empty_template_duplicates_and_a_shared_pair(world):
    dev, tset, piv, vols = world["dev"], world["tset"], world["piv"], world["vols"]
    rng = np.random.default_rng(3)
    jobs = [(1, 0, 1, -199, -190, 256, 256), (2, 0, N, -120, -100, 128, 64), (3, 5, 4, -120, -150, 128, 128),  # 65 536 points
            (0, 0, N, -60, -50, 9, 9), (0, 2, 1, -199, -190, 256, 256),                                         # no lines
            (2, 1, 3, -64, -50, 5, 5), (2, 1, 3, -64, -50, 5, 5), (1, 0, 1, -199, -190, 256, 256)]               # duplicates
    jobs += [(2, 1, 1, int(rng.integers(-150, 40)), int(rng.integers(-180, 60)), 3, 3) for _ in range(300)]       # one (tmpl, a)
    jobs = np.asarray(jobs, dtype=np.int32)
    for k in (1, 64):
        got = dev.exhaustive_window_search(tset, jobs, CS, piv, wrap=True, k=k)
        _same(got, window_records(vols, MASTER, jobs, CS, piv, k, 1, 1, True))
    rec, off = got
    assert off[1] == 64 and off[4] == off[3] == off[5] and off[3] - off[2] == 64
    assert rec[off[5]:off[6]].tobytes() == rec[off[6]:off[7]].tobytes() and off[6] - off[5] == 64
    assert rec[:64].tobytes() == rec[off[7]:off[8]].tobytes()
    assert 0 < (np.diff(off)[8:] == 9).sum() < 300  # 3 x 3 windows, k = 64: count < k, some across an edge or outside


def test_identity_with_the_rotation_search_job_by_job(world):
    """The definition: each job's records are fdcm_search_exhaustive_rotations' on the one-template set, with the run's
    rotations in run order, the job's grid, radii 0 and base tmpl + tmpl_index_base."""
    from openfdcm_amd.engine import DeviceTemplates
    dev, tset, piv, tmpls = world["dev"], world["tset"], world["piv"], world["tmpls"]
    one = [DeviceTemplates([tm]) for tm in tmpls]
    for (sx, sy), k in [((1, 1), 8), ((4, 2), 64)]:
        jobs = _jobs(sx, sy, True)[::5]
        jobs = np.concatenate([jobs, np.int32([(0, 1, 2, -60, -50, 3, 3)])])
        rec, off = dev.exhaustive_window_search(tset, jobs, CS, piv, sx=sx, sy=sy, wrap=True, k=k, tmpl_index_base=-2)
        assert len(rec) > 100
        for j, (t, a0, na, x0, y0, nx, ny) in enumerate(jobs):
            run = (a0 + np.arange(na)) % N
            want = dev.exhaustive_rotation_search(one[t], (x0, y0, nx, ny, sx, sy), CS[run], piv[t:t + 1], k=k, tmpl_index_base=t - 2)
            assert rec[off[j]:off[j + 1]].tobytes() == want.tobytes(), j


def test_translations_only_is_the_translation_search(world):
    """rot = NULL: the caller's lines as they are -- the last template has a line from x = +0 to x = -0, whose x2 - x1 is
    -0 and whose angle is atan(-inf); an identity rotation would make both +0 and the angle atan(+inf) -- and
    fdcm_search_exhaustive's literal records."""
    from openfdcm_amd.engine import DeviceTemplates
    dev, vols0, tmpls = world["dev"], world["vols0"], world["tmpls"]
    neg = np.array([[0.0, 30.0, -0.0, 90.0], [40.0, 0.0, 100.0, -0.0], [-0.0, -0.0, 60.0, 50.0]], dtype=np.float32).T.copy()
    tm2 = list(tmpls) + [neg]
    T = len(tmpls)
    tset = DeviceTemplates(tm2)
    extra = [(T, 0, 1, -20 + r, 3, nx, ny) for r in range(4) for nx, ny in WINDOWS] + [(0, 0, 1, 0, 0, 5, 5)]
    for (sx, sy), k in [((1, 1), 1), ((1, 1), 64), ((2, 3), 8)]:
        jobs = _jobs(sx, sy, False)[::3].copy()
        jobs[:, 1], jobs[:, 2] = 0, 1
        jobs = np.concatenate([jobs, np.int32(extra)])
        rec, off = dev.exhaustive_window_search(tset, jobs, None, None, sx=sx, sy=sy, k=k, tmpl_index_base=3)
        inside = jobs[:, 0] < T
        wrec, woff = window_records(list(vols0) + [None], MASTER, jobs[inside], None, None, k, sx, sy, False, base=3)
        assert np.array_equal(np.diff(off)[inside], np.diff(woff)) and len(wrec) > 20
        for q, j in enumerate(np.nonzero(inside)[0]):
            assert rec[off[j]:off[j + 1]].tobytes() == wrec[woff[q]:woff[q + 1]].tobytes(), j
        assert np.all(rec["transform"][:, [0, 1, 3, 4]] == [1, 0, 0, 1]) and not np.signbit(rec["transform"][:, 1]).any()
        one = [DeviceTemplates([tm]) for tm in tm2]
        for j in np.nonzero(~inside | (np.arange(len(jobs)) % 7 == 0))[0]:
            t, a0, na, x0, y0, nx, ny = jobs[j]
            w = dev.exhaustive_search(one[t], (x0, y0, nx, ny, sx, sy), k=k, tmpl_index_base=t + 3)
            assert rec[off[j]:off[j + 1]].tobytes() == w.tobytes(), j
        assert off[-1] - off[-2] == 0 and off[-2] - off[-3] > 0  # the template without lines; the -0 template scores


def _adopted_scores(vol, lines, xs, ys):
    """evaluate on an adopted one-slice volume with scene translation 0 for a template of fewer than 4 lines (the scalar
    tail: a running float32 sum in line order): (len(ys), len(xs)) float32, NaN where not admissible."""
    W, H = vol.shape
    out = np.full((len(ys), len(xs)), np.nan, dtype=np.float32)
    for jj, ty in enumerate(ys):
        for ii, tx in enumerate(xs):
            p = lines + np.float32([tx, ty, tx, ty])[:, None]
            if not (np.all(p[[0, 2]] > -1) and np.all(p[[0, 2]] < W) and np.all(p[[1, 3]] > -1) and np.all(p[[1, 3]] < H)):
                continue
            q = p.astype(np.int32)
            s = np.float32(0)
            with np.errstate(invalid="ignore"):
                for l in range(lines.shape[1]):
                    s = np.float32(s + np.abs(vol[q[0, l], q[1, l]] - vol[q[2, l], q[3, l]]))
            out[jj, ii] = s
    return out


def test_all_zero_volume_ties_order_by_run_position_then_grid_index():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy()]
    tset = DeviceTemplates(tmpls)
    cs = _cs([0, 90, 180, 270, 30])
    piv = _centers(tmpls)
    master = (-30, -30, 70, 70)
    rs = rotated_set(tmpls, cs, piv)
    vol = np.stack([np.where(admissible_mask(l, (0.0, 0.0), 40, 30, master), np.float32(0), np.float32(np.nan)) for l in rs])
    jobs = np.int32([(0, 0, 5, -25, -24, 30, 31), (0, 3, 4, 2, 2, 7, 5), (0, 4, 1, 0, 0, 1, 1), (0, 2, 2, -30, -30, 70, 70)])
    for k in (1, 9, 64):
        got = dev.exhaustive_window_search(tset, jobs, cs, piv, wrap=True, k=k)
        assert np.all(got[0]["score"] == 0) and len(got[0]) > 2 * k
        _same(got, window_records([vol], master, jobs, cs, piv, k, 1, 1, True))
    rec, off = got
    run = [3, 4, 0, 1]  # job 1: all scores tie, so its records come run position by run position, rotation 3 first
    pos = [[e for e, a in enumerate(run) if r["transform"][0] == cs[a, 0] and r["transform"][3] == cs[a, 1]][0] for r in rec[off[1]:off[2]]]
    assert pos[0] == 0 and pos == sorted(pos) and len(set(pos)) >= 2


def test_adopted_volume_with_a_nan_and_an_infinity():
    """A NaN score has no key; an infinite one is kept and orders last; inf - inf is NaN."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    rng = np.random.default_rng(11)
    vol = rng.integers(0, 50, size=(24, 20)).astype(np.float32)
    vol[7, 9] = np.nan
    vol[15, 4] = np.inf
    vol[16, 12] = np.inf
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), vol[None], (0.0, 0.0))
    tmpls = [np.array([[1, 2, 6, 2], [3, 1, 3, 8], [0, 0, 1, 8]], dtype=np.float32).T.copy(),
             np.array([[15 - 16, 4 - 12, 0, 0]], dtype=np.float32).T.copy()]  # joins the two infinities at t = (16, 12)
    tset = DeviceTemplates(tmpls)
    xs, ys = np.arange(-4, 26), np.arange(-4, 22)
    vols = [_adopted_scores(vol, tm, xs, ys)[None] for tm in tmpls]
    assert np.isinf(vols[0]).sum() >= 4 and (np.isnan(vols[0]) & admissible_mask(tmpls[0], (0, 0), 24, 20, (-4, -4, 30, 26))).sum() >= 3
    assert np.isnan(vols[1][0, 12 + 4, 16 + 4])  # inf - inf
    jobs = np.int32([(0, 0, 1, -4, -4, 30, 26), (0, 0, 1, 5, 2, 9, 9), (1, 0, 1, 12, 8, 9, 9), (1, 0, 1, -4, -4, 30, 26),
                     (0, 0, 1, 12, 0, 3, 17)])
    for k in (8, 64):
        for cs in (None, np.float32([[1, 0]])):
            got = dev.exhaustive_window_search(tset, jobs, cs, None, k=k)
            want = window_records(vols, (-4, -4, 30, 26), jobs, cs, None, k, 1, 1, False)
            _same(got, want)
    assert not np.isnan(got[0]["score"]).any() and np.isinf(got[0]["score"]).any()


def _probe(env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "windows_probe.py")], capture_output=True, text=True,
                         timeout=300, env={**{k: v for k, v in os.environ.items() if not k.startswith("FDCM_WINDOWS")}, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("windows_probe ")][-1].split()
    return line[1], int(line[3])


def test_batches_and_flat_addresses_give_the_same_bytes():
    """In fresh processes (the switches are read once): batches of 5 planes at most -- the probe's 72 jobs hold more than 200
    planes, so dozens of batches, each job with more than 5 planes a batch of its own, and with the switch the list also
    goes in rounds of 20 KB of tables, an upload and a download each -- and the 64-bit addressing form."""
    spec = __import__("importlib.util").util.spec_from_file_location("windows_probe", os.path.join(ROOT, "tools", "windows_probe.py"))
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    calls = probe.case()[4]
    assert calls[0][0][:, 2].sum() >= 3 * 5 * 10
    default = _probe({})
    assert default[1] > 1000
    assert _probe({"FDCM_WINDOWS_BATCH": "5"}) == default
    assert _probe({"FDCM_WINDOWS_FLAT": "1"}) == default
    if not any(k.startswith("FDCM_WINDOWS") for k in os.environ):
        assert probe.run() == default


def test_public_api_refines_a_planted_pose():
    """A shape planted at 90 degrees and t = (81, 70); the coarse table (every 20 degrees) and grid (stride 4) hold neither.
    The best coarse peak is within 10 degrees and 3 pixels, and the best refined pose is the planted one at score 0."""
    import openfdcm_amd as openfdcm
    S = 200
    shape = np.array([(0, 0, 60, 0), (60, 0, 60, 45), (0, 0, 0, 70), (0, 70, 35, 70), (35, 70, 35, 45), (35, 45, 60, 45)],
                     dtype=np.float32).T.copy()
    fine = np.deg2rad(np.arange(360))
    coarse = np.deg2rad(np.arange(0, 360, 20))
    c, s = np.float32(np.cos(fine[90])), np.float32(np.sin(fine[90]))
    inst = rotate_lines(shape, c, s, 30, 35) + np.float32([81, 70, 81, 70])[:, None]
    frame = np.array([(0, 0, S / 8, 0), (S - 1, S - 1, S - 1 - S / 8, S - 1), (20, 150, 70, 190), (150, 20, 190, 60)], dtype=np.float32).T
    scene = np.concatenate([frame, inst], axis=1).astype(np.float32)
    fm = openfdcm.build_cpu_featuremap(scene, openfdcm.Dt3CpuParameters(depth=12, dt3Coeff=5.0, padding=1.0))
    tmpls = [shape]
    piv = openfdcm.template_pivots(tmpls)
    assert piv.tolist() == [[30, 35]]
    seeds = openfdcm.exhaustive_rotation_search(fm, tmpls, coarse, stride=4, k=4, radius=2, angle_radius=1, wrap=True)
    assert len(seeds) == 4 and seeds[0].score > 100
    jobs = openfdcm.pose_windows(seeds, coarse, fine, piv, 12, 6, 6)
    assert jobs.shape == (4, 7) and jobs[0].tolist() == [0, 68, 25, 78, 62, 13, 13]
    refined, offsets = openfdcm.exhaustive_window_search(fm, tmpls, jobs, angles=fine, k=3)
    assert offsets.tolist() == [0, 3, 6, 9, 12] and len(refined) == 12
    best = refined[0]
    assert best.tmpl_idx == 0 and best.score == 0 and refined[1].score > 0
    tr = np.asarray(best.transform)
    assert tr[0, 0] == c and tr[1, 0] == s
    m = np.float32([30, 35]) - np.float32([c * np.float32(30) + (-s) * np.float32(35), s * np.float32(30) + c * np.float32(35)])
    assert tr[0, 2] == m[0] + np.float32(81) and tr[1, 2] == m[1] + np.float32(70)
    again = openfdcm.pose_windows(refined[:1], fine, fine, piv, 0, 0, 0)
    assert again.tolist() == [[0, 90, 1, 81, 70, 1, 1]]
    # tracking: translations only, around the last frame's positions
    tr_jobs = np.int32([(0, 0, 1, -5, -5, 11, 11)])
    t_only, off = openfdcm.exhaustive_window_search(fm, tmpls, tr_jobs, k=2)
    assert len(t_only) == 2 and np.array_equal(np.asarray(t_only[0].transform)[:, :2], np.eye(2))


def test_bad_arguments_then_a_valid_call(world):
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates, _rotations
    dev, tset, piv = world["dev"], world["tset"], world["piv"]
    good = np.int32([(1, 6, 4, -60, -50, 9, 9), (3, 0, 1, -110, -60, 17, 65)])
    want = dev.exhaustive_window_search(tset, good, CS, piv, wrap=True, k=5)
    assert len(want[0]) == 10
    bad_piv = piv.copy()
    bad_piv[2, 0] = np.inf

    def call(jobs, cs=CS, pv=piv, sx=1, sy=1, wrap=1, k=5):
        jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 7)
        rot, keep = _rotations(cs, pv, tset.count)
        out, n = C.c_void_p(), C.c_int64(-7)
        off = np.full(len(jobs) + 1, -7, dtype=np.int64)
        return capi.lib().fdcm_search_exhaustive_windows(dev._h, tset._h, C.byref(rot), jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)),
                                                         len(jobs), sx, sy, wrap, k, 0, C.byref(out), C.byref(n),
                                                         off.ctypes.data_as(C.POINTER(C.c_int64)))

    cases = [dict(jobs=[(len(LINES), 0, 1, 0, 0, 3, 3)]), dict(jobs=[(1, 0, 1, 0, 0, 3, 3), (-1, 0, 1, 0, 0, 3, 3)]),
             dict(jobs=good, wrap=0), dict(jobs=[(1, 0, 9, 0, 0, 3, 3)]), dict(jobs=[(1, 8, 1, 0, 0, 3, 3)]),
             dict(jobs=[(1, 0, 1, 0, 0, 0, 3)]), dict(jobs=[(1, 0, 2, 0, 0, 256, 129)]), dict(jobs=[(1, 0, 1, 1 << 24, 0, 3, 3)]),
             dict(jobs=good, sx=0), dict(jobs=good, k=65), dict(jobs=good, k=0), dict(jobs=good, wrap=2),
             dict(jobs=good, cs=np.float32([[1, np.nan]] * N)), dict(jobs=good, pv=bad_piv)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert capi.lib().fdcm_last_error()
        got = dev.exhaustive_window_search(tset, good, CS, piv, wrap=True, k=5)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    # the edge cases: no jobs, an empty map, an empty template list -- zero records, offsets all 0
    rec, off = dev.exhaustive_window_search(tset, np.zeros((0, 7), np.int32), CS, piv)
    assert len(rec) == 0 and off.tolist() == [0]
    empty = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    rec, off = empty.exhaustive_window_search(tset, good, CS, piv, wrap=True, k=5)
    assert len(rec) == 0 and off.tolist() == [0, 0, 0]
    rec, off = dev.exhaustive_window_search(DeviceTemplates([]), good, CS, None, wrap=True, k=5)
    assert len(rec) == 0 and off.tolist() == [0, 0, 0]
