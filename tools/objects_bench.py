"""Times the detector with objects (include/fdcm.h, "Objects") against the calls that were there, on config 2' (bench.py's
feature map and its 1000 x 32-line synthetic templates), line caps 3, ExponentialPenalty(1.5), overlap 0.3, max_detections 64:

  dense      per stride (1, 2, 4) on the default window, at max_score = +inf:
               detect_all       exhaustive_detect_all, the call every build has (the yardstick, and its own spread)
               objects_G        exhaustive_detect_objects with G = 1, 4, 16 objects, templates dealt round-robin, cross limit
                                equal to the overlap limit (builds that have the call)
               composed_G       what was available before for G = 4, 16: one exhaustive_detect_all per object on that object's
                                templates, and the cross-object rule in numpy on the downloaded lists
  windows    tools/window_detect_bench.py's refinement workload (100 templates, 800 seeds, boxes of 11 x 9 x 9 poses on a table
             of 360 angles): exhaustive_detect_windows, and exhaustive_detect_windows_objects with 4 objects

Each figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.  One process measures
one build (--package-root: the directory that holds its openfdcm_amd; this checkout by default).  With --parent DIR the tool
runs itself as processes in turn, the build under DIR and this one, --rounds times each, and writes all of it to --json: a
difference between detect_all of the parent and objects_1 of this build is read against the spread of the parent's own runs.

    python tools/objects_bench.py [--reps 5] [--strides 1,2,4] [--objects 1,4,16] [--skip-windows] [--package-root DIR] [--json out.json]
    python tools/objects_bench.py --parent DIR [--rounds 2] --json profiles/objects_bench_config2p.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def cross_rule(lists, permille, k):
    """The cross-object rule on downloaded lists, in numpy: lists[o] = (records, boxes) of object o, each already suppressed
    within its object.  Greedy by (score bits, object order), a detection dropping the records of other objects whose boxes
    overlap its own by more than permille / 1000; at most k.  Returns the number kept."""
    rec = np.concatenate([r for r, _ in lists])
    box = np.concatenate([b for _, b in lists]).astype(np.int64)
    obj = np.concatenate([np.full(len(r), o) for o, (r, _) in enumerate(lists)])
    order = np.argsort(rec["score"].view(np.uint32), kind="stable")
    area = (box[:, 2] - box[:, 0] + 1) * (box[:, 3] - box[:, 1] + 1)
    left = np.ones(len(rec), dtype=bool)
    kept = 0
    for d in order:
        if not left[d]:
            continue
        kept += 1
        if kept == k:
            break
        w = np.maximum(0, np.minimum(box[:, 2], box[d, 2]) - np.maximum(box[:, 0], box[d, 0]) + 1)
        h = np.maximum(0, np.minimum(box[:, 3], box[d, 3]) - np.maximum(box[:, 1], box[d, 1]) + 1)
        inter = w * h
        left &= ~((obj != obj[d]) & (1000 * inter > permille * (area + area[d] - inter)))
    return kept


def measure(args):
    sys.path.insert(0, os.path.abspath(args.package_root))
    import openfdcm_amd as openfdcm
    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates

    has = hasattr(DeviceFeatureMap, "exhaustive_detect_objects")
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    pm = int(round(1000 * args.overlap))
    Gs = [int(v) for v in args.objects.split(",") if v]
    res = {"package": os.path.relpath(os.path.abspath(args.package_root), ROOT), "has_objects": has, "line_caps": args.line_caps,
           "overlap_permille": pm, "dense": [], "windows": None}
    tset = DeviceTemplates(tmpls, line_caps=args.line_caps)
    pen, tau = _capi.EXPONENTIAL_PENALTY, args.tau
    T = len(tmpls)
    for s in [int(v) for v in args.strides.split(",") if v]:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        row = {"stride": s, "grid": list(grid), "grid_points": grid[2] * grid[3]}
        out, t = timed(lambda: dev.exhaustive_detect_all(tset, grid, max_detections=64, overlap_permille=pm, penalty=pen, tau=tau, boxes=True),
                       args.reps)
        t["detections"] = int(len(out[0]))
        row["detect_all"] = t
        print(f"dense stride {s} detect_all: {t}", flush=True)
        for G in Gs:
            obj = np.arange(T, dtype=np.int32) % G
            if has:
                out, t = timed(lambda: dev.exhaustive_detect_objects(tset, grid, obj, float("inf"), G, max_detections=64, overlap_permille=pm,
                                                                     cross_permille=pm, penalty=pen, tau=tau, boxes=True), args.reps)
                t["detections"] = int(len(out[0]))
                row[f"objects_{G}"] = t
                print(f"dense stride {s} objects_{G}: {t}", flush=True)
            if G > 1:
                subs = [DeviceTemplates([tmpls[i] for i in range(T) if obj[i] == o], line_caps=args.line_caps) for o in range(G)]

                def composed():
                    lists = [dev.exhaustive_detect_all(sub, grid, max_detections=64, overlap_permille=pm, penalty=pen, tau=tau, boxes=True)
                             for sub in subs]
                    return cross_rule(lists, pm, 64)
                out, t = timed(composed, args.reps)
                t["detections"] = int(out)
                row[f"composed_{G}"] = t
                print(f"dense stride {s} composed_{G}: {t}", flush=True)
        res["dense"].append(row)

    if not args.skip_windows:
        sub = tmpls[:100]
        wset = DeviceTemplates(sub, line_caps=args.line_caps)
        piv = openfdcm.template_pivots(sub)
        coarse, fine = np.arange(36) * (2 * np.pi / 36), np.arange(360) * (2 * np.pi / 360)
        ccs, fcs = openfdcm._angles(coarse), openfdcm._angles(fine)
        P = _capi.DEFAULT_PENALTY
        grid = dev.exhaustive_rotations_window(wset, ccs, piv, 4, 4).as_tuple()
        seeds = dev.exhaustive_detect_all(wset, grid, ccs, piv, max_detections=800, overlap_permille=1000, penalty=P)
        jobs = openfdcm.pose_windows(seeds, coarse, fine, piv, 5, 4, 4, wrap=True)
        row = {"jobs": int(len(jobs)), "box": [int(jobs[0, 2]), int(jobs[0, 5]), int(jobs[0, 6])]}
        out, t = timed(lambda: dev.exhaustive_detect_windows(wset, jobs, fcs, piv, wrap=True, max_detections=1024, overlap_permille=pm,
                                                             penalty=P, boxes=True, job_index=True), args.reps)
        t["detections"] = int(len(out[0]))
        row["detect_windows"] = t
        print(f"windows detect_windows: {t}", flush=True)
        if has:
            obj = np.arange(len(sub), dtype=np.int32) % 4
            out, t = timed(lambda: dev.exhaustive_detect_windows_objects(wset, jobs, obj, float("inf"), 4, fcs, piv, wrap=True,
                                                                         max_detections=1024, overlap_permille=pm, cross_permille=pm,
                                                                         penalty=P, boxes=True, job_index=True), args.reps)
            t["detections"] = int(len(out[0]))
            row["objects_4"] = t
            print(f"windows objects_4: {t}", flush=True)
        res["windows"] = row
    return res


def compare(args):
    """The parent's build and this one as processes in turn, --rounds times each."""
    runs = []
    for r in range(args.rounds):
        for who, root in (("parent", args.parent), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", root, "--reps", str(args.reps), "--strides", args.strides,
                   "--objects", args.objects, "--line-caps", str(args.line_caps), "--overlap", str(args.overlap),
                   "--tau", str(args.tau)] + (["--skip-windows"] if args.skip_windows else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
            if out.returncode != 0:
                raise SystemExit(f"{who} (round {r}) failed:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
            res = json.loads(out.stdout.strip().splitlines()[-1])
            res["build"], res["round"] = who, r
            runs.append(res)
            print(f"round {r}: {who} done", flush=True)
    return {"workload": "config 2': 1024x1024 scene (200 lines, seed 1), depth 30, L2, padding 1.0; dense: 1000 templates x 32 lines "
                        "(seed 2) dealt round-robin to G objects, default window per stride, ExponentialPenalty(%g), max_detections 64; "
                        "windows: 100 templates, 800 seeds, 11 x 9 x 9 poses of 360 angles, DefaultPenalty, max_detections 1024" % args.tau,
            "runs": runs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--strides", default="1,2,4")
    ap.add_argument("--objects", default="1,4,16")
    ap.add_argument("--tau", type=float, default=1.5)
    ap.add_argument("--line-caps", type=float, default=3.0)
    ap.add_argument("--overlap", type=float, default=0.3)
    ap.add_argument("--skip-windows", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", default=None, help="a directory that holds the parent commit's built openfdcm_amd")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = compare(args) if args.parent else measure(args)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
