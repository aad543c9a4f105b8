"""Times refine_matches (include/fdcm.h, "Match lists: refinement") on one GPU, on the records of one config-2' frame as
tools/match_detect_bench.py sets it up (1024 x 1024, 200 scene lines, 1000 templates of 32 lines, DefaultSearch(4, 4),
BatchOptimize(10): about 27 000 records), delta_angles(5, 1 degree), half_x = half_y = 4, stride 1, pivot "center", no caps:

  refine host / device / last   refine_matches on host records, on the same records in a device buffer, and on the records of
                                the last search (matches=None); the records come back to the host in all three
  composition                   what a caller had before: the lines of every (record, delta) posed in numpy and
                                fdcm_featuremap_evaluate at the window's translations, the keys and the winner in numpy; one
                                run; the tool fails unless it returns the same bytes
  detect_matches                the call both builds have (the yardstick: this build's figure is read against the parent's
                                processes, the machine code being the same): DefaultPenalty, overlap 0.3, max_detections 64

Each figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.  One process measures
one build (--package-root).  With --parent DIR the tool runs itself as processes in turn, the build under DIR and this one,
--rounds times each, and writes all of it to --json.

    python tools/refine_bench.py [--reps 5] [--package-root DIR] [--json out.json]
    python tools/refine_bench.py --parent DIR [--rounds 2] --json profiles/refine_bench_config2p.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_STEPS, STEP, HALF = 5, np.deg2rad(1.0), 4
RULE = dict(overlap=0.3, max_detections=64)
f32 = np.float32


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def composition(openfdcm, fm, tmpls, rec, angles, chunk=4096):
    """(records, poses) of refine_matches by numpy posing and fdcm_featuremap_evaluate, `chunk` records a call; templates of one
    line count, no caps."""
    parts = [composition_part(openfdcm, fm, tmpls, rec[q:q + chunk], angles) for q in range(0, len(rec), chunk)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def composition_part(openfdcm, fm, tmpls, rec, angles):
    from openfdcm_amd import _capi
    dev = fm._fm
    n, na, nw = len(rec), len(angles), 2 * HALF + 1
    N = nw * nw
    cs = openfdcm._angles(angles)
    pv = openfdcm._pivots(tmpls, "center", len(tmpls))
    L = np.stack([np.asarray(t, dtype=np.float32).reshape(4, -1) for t in tmpls])          # (T, 4, nl)
    nl = L.shape[2]
    ti = rec["tmpl_idx"].astype(np.int64)
    M = rec["transform"].astype(np.float32)
    planes = np.empty((n, na, nl, 4), dtype=np.float32)
    mxy = np.empty((na, len(tmpls), 2), dtype=np.float32)
    for e, (c, s) in enumerate(cs):
        ns = -s
        px, py = pv[:, 0], pv[:, 1]
        mx, my = px - (c * px + ns * py), py - (s * px + c * py)                              # rot_matrix, float32, unfused
        mxy[e, :, 0], mxy[e, :, 1] = mx, my
        for a in (0, 2):
            qx = (c * L[:, a] + ns * L[:, a + 1]) + mx[:, None]                              # Q_e(t): (T, nl)
            qy = (s * L[:, a] + c * L[:, a + 1]) + my[:, None]
            x, y = qx[ti], qy[ti]                                                            # (n, nl)
            planes[:, e, :, a] = (M[:, 0:1] * x + M[:, 1:2] * y) + M[:, 2:3]
            planes[:, e, :, a + 1] = (M[:, 3:4] * x + M[:, 4:5] * y) + M[:, 5:6]
    P = n * na
    offsets = np.arange(P + 1, dtype=np.int64) * nl
    d = np.arange(-HALF, HALF + 1, dtype=np.float32)
    win = np.stack([np.tile(d, nw), np.repeat(d, nw)], axis=1)                               # g = (j + h) nw + (i + h)
    trs = np.ascontiguousarray(np.broadcast_to(win, (P, N, 2))).reshape(-1, 2)
    toff = np.arange(P + 1, dtype=np.int64) * N
    scores = np.zeros(P * N, dtype=np.float32)
    flat = np.ascontiguousarray(planes.reshape(-1, 4))
    _capi.check(_capi.lib().fdcm_featuremap_evaluate(dev._h, _capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), P, _capi.fptr(trs),
                                                      toff.ctypes.data_as(C.POINTER(C.c_int64)), _capi.fptr(scores)))
    scores = scores.reshape(n, na * N)
    low = 1 + np.arange(na * N, dtype=np.uint64)
    centre = HALF_STEPS * N + HALF * nw + HALF
    low[centre] = 0
    keys = (scores.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[None, :]
    keys[np.isnan(scores)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.argmin(keys, axis=1)
    kmin = keys[np.arange(n), best]
    won = kmin != np.uint64(0xFFFFFFFFFFFFFFFF)
    e, g = best // N, best % N
    i, j = (g % nw - HALF).astype(np.int32), (g // nw - HALF).astype(np.int32)
    out = np.array(rec)
    out["score"] = np.where(won, scores[np.arange(n), best], f32(np.nan))
    c, s = cs[e, 0], cs[e, 1]
    ns = -s
    mx, my = mxy[e, ti, 0], mxy[e, ti, 1]
    T = np.stack([(M[:, 0] * c + M[:, 1] * s), (M[:, 0] * ns + M[:, 1] * c), ((M[:, 0] * mx + M[:, 1] * my) + M[:, 2]) + i.astype(np.float32),
                  (M[:, 3] * c + M[:, 4] * s), (M[:, 3] * ns + M[:, 4] * c), ((M[:, 3] * mx + M[:, 4] * my) + M[:, 5]) + j.astype(np.float32)],
                 axis=1).astype(np.float32)
    out["transform"] = np.where(won[:, None], T, M)
    pose = np.stack([np.where(won, e, -1), np.where(won, i, 0), np.where(won, j, 0)], axis=1).astype(np.int32)
    return out, pose


def canon(rec):
    """The records with every NaN as the one quiet NaN."""
    rec = np.array(rec)
    for k in ("score", "transform"):
        rec[k][np.isnan(rec[k])] = f32(np.nan)
    return rec.tobytes()


def measure(args):
    sys.path.insert(0, os.path.abspath(args.package_root))
    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic

    has = hasattr(openfdcm, "refine_matches")
    cfg, scene, tmpls = synthetic.make_config("2p")
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0, padding=1.0, distance=openfdcm.distance(cfg["distance"]))
    fm = openfdcm.build_cpu_featuremap(scene, params)
    matches = openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(4, 4), openfdcm.BatchOptimize(10), fm, tmpls, scene)
    rec = np.array(matches.records())
    pen = openfdcm.DefaultPenalty()
    res = {"package": os.path.relpath(os.path.abspath(args.package_root), ROOT), "has_refine": has, "records": len(rec)}
    _, res["detect_matches"] = timed(lambda: openfdcm.detect_matches(fm, tmpls, matches, penalty=pen, **RULE), args.reps)
    print("detect_matches", res["detect_matches"], flush=True)
    if not has:
        return res
    angles = openfdcm.delta_angles(HALF_STEPS, STEP)
    kw = dict(angles=angles, half_x=HALF, half_y=HALF, return_poses=True)
    hip = C.CDLL("libamdhip64.so")  # (the runtime the library has loaded): a device buffer with the records
    buf = C.c_void_p()
    if hip.hipMalloc(C.byref(buf), C.c_size_t(rec.nbytes)) != 0 or hip.hipMemcpy(buf, C.c_void_p(rec.ctypes.data), C.c_size_t(rec.nbytes), 1) != 0:
        sys.exit("no device buffer for the records")
    calls = {"refine_host": lambda: openfdcm.refine_matches(fm, tmpls, matches, **kw),
             "refine_device": lambda: openfdcm.refine_matches(fm, tmpls, None, device_ptr=buf.value, n=len(rec), **kw),
             "refine_last_search": lambda: openfdcm.refine_matches(fm, tmpls, None, **kw)}
    outs = {}
    for name, call in calls.items():
        outs[name], res[name] = timed(call, args.reps)
        print(name, res[name], flush=True)
    got, pose = outs["refine_host"]
    won = pose[:, 0] >= 0
    res["winners"] = int(won.sum())
    res["moved"] = int((won & np.any(pose != (HALF_STEPS, 0, 0), axis=1)).sum())
    res["lookups"] = int(won.sum()) * len(angles) * (2 * HALF + 1) ** 2 * 32 * 2
    res["forms_identical"] = bool(all(canon(o[0].records()) == canon(got.records()) and np.array_equal(o[1], pose) for o in outs.values()))
    first = openfdcm.detect_matches(fm, tmpls, matches, penalty=pen, **RULE)
    after = openfdcm.detect_matches(fm, tmpls, got, penalty=pen, **RULE)
    res["detections_before"], res["detections_after_refine"] = len(first), len(after)
    t0 = time.perf_counter()
    want, wpose = composition(openfdcm, fm, tmpls, rec, angles)
    res["composition"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "runs": 1}
    print("composition", res["composition"], flush=True)
    res["identical_to_composition"] = bool(canon(want) == canon(got.records()) and np.array_equal(wpose, pose))
    hip.hipFree(buf)
    if not (res["identical_to_composition"] and res["forms_identical"]):
        print(json.dumps(res))
        sys.exit("the call and the composition of the calls before it differ, or the three forms do")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", default=None, help="the parent commit's checkout, built: processes of both builds in turn")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.parent is None:
        res = measure(args)
        print("RESULT " + json.dumps(res), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    runs = []
    for r in range(args.rounds):
        for root in (args.parent, ROOT):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--package-root", root], capture_output=True,
                                 text=True, timeout=900)
            if out.returncode != 0:
                sys.exit(out.stdout + out.stderr)
            runs.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(runs[-1]["package"], {k: v for k, v in runs[-1].items() if k.startswith(("detect", "refine", "composition"))}, flush=True)
    res = {"workload": "the records of one config-2' frame (1024 x 1024, 200 scene lines, 1000 templates of 32 lines, DefaultSearch(4, 4), "
                       "BatchOptimize(10)); delta_angles(5, 1 degree), half_x = half_y = 4, stride 1, pivot \"center\", no caps: 11 x 9 x 9 poses "
                       "per record; detect_matches: DefaultPenalty, overlap 0.3, max_detections 64",
           "protocol": f"median of {args.reps} blocking calls after a warm-up, host wall clock, the records returned to the host; processes in "
                       f"turn, the parent's build and this one, {args.rounds} each",
           "runs": runs,
           "not_measured": ["the kernels' own times (no rocprofv3 --kernel-trace run)", "HBM traffic and counters (no --pmc run)",
                            "lists above one frame's records, and a list in more than one part", "templates above 32 lines", "line caps",
                            "windows above 11 x 9 x 9", "the host-libm path", "records left on the device (out_device_ptr)",
                            "more than one GPU"]}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
