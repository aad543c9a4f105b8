"""Times the matched-fraction gate of the detector where it is applied (include/fdcm.h, "Gate inside the minimum") on config
2' (bench.py's feature map and its 1000 x 32-line synthetic templates), line caps 3, ExponentialPenalty(1.5), overlap 0.3:

  dense      exhaustive_detect_all(min_matched = m) on the default window at strides 1, 2 and 4, max_detections 64, at
             max_score = +inf and at the 5 % quantile of the best map's finite scores: gate WINNER (the call every build since
             the gate has) and, where the build has it, gate ALL
  windows    exhaustive_detect_windows(min_matched = m) on tools/window_detect_bench.py's refinement workload (100 templates,
             800 seeds of the coarse stage, boxes of 11 x 9 x 9 poses on a table of 360 angles): gate WINNER and gate ALL

m is 0.26 by default, the median fraction of the ungated detections of this workload (README, "Detections by matched
fraction"), so that the gate keeps something.  Each figure is the median of --reps blocking calls after a warm-up, with the
smallest and the largest.

One process measures one build (--package-root: the directory that holds its openfdcm_amd; this checkout by default).  With
--parent DIR the tool runs itself as processes in turn, the build under DIR and this one, --rounds times each (2 by
default), and writes all of it to --json: the existing call of this build must stay within the spread of the parent's own
runs; what gate ALL costs or saves is read against that spread.

    python tools/detect_gate_bench.py [--reps 5] [--strides 1,2,4] [--skip-windows] [--package-root DIR] [--json out.json]
    python tools/detect_gate_bench.py --parent DIR [--rounds 2] --json profiles/detect_gate_bench_config2p.json
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


def measure(args):
    sys.path.insert(0, os.path.abspath(args.package_root))
    import inspect

    import openfdcm_amd as openfdcm
    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates

    has_gate = "gate" in inspect.signature(DeviceFeatureMap.exhaustive_detect_all).parameters
    gates = ["winner"] + (["all"] if has_gate else [])
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    pm, m = int(round(1000 * args.overlap)), args.min_matched
    res = {"package": os.path.relpath(os.path.abspath(args.package_root), ROOT), "has_gate_all": has_gate, "min_matched": m, "line_caps": args.line_caps,
           "overlap_permille": pm, "dense": [], "windows": None}

    tset = DeviceTemplates(tmpls, line_caps=args.line_caps)
    pen, tau = _capi.EXPONENTIAL_PENALTY, args.tau
    for s in [int(v) for v in args.strides.split(",") if v]:
        grid = dev.exhaustive_window(tset, s, s).as_tuple()
        scores, _ = dev.best_map(tset, grid, penalty=pen, tau=tau)
        fin = np.sort(scores[np.isfinite(scores)])
        row = {"stride": s, "grid": list(grid), "grid_points": grid[2] * grid[3]}
        for name, ms in [("inf", float("inf")), ("q5", float(fin[min(len(fin) - 1, int(0.05 * len(fin)))]))]:
            for gate in gates:
                kw = {"gate": gate} if has_gate else {}
                out, t = timed(lambda: dev.exhaustive_detect_all(tset, grid, max_score=ms, max_detections=64, overlap_permille=pm, penalty=pen,
                                                                 tau=tau, min_matched=m, matched=True, **kw), args.reps)
                t.update({"max_score": ms, "detections": int(len(out[0])),
                          "fraction_min_median": [round(float(out[1].min()), 4), round(float(np.median(out[1])), 4)] if len(out[0]) else []})
                row[f"{name}_{gate}"] = t
                print(f"dense stride {s} max_score {name} gate {gate}: {t}", flush=True)
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
        for gate in gates:
            kw = {"gate": gate} if has_gate else {}
            out, t = timed(lambda: dev.exhaustive_detect_windows(wset, jobs, fcs, piv, wrap=True, max_detections=1024, overlap_permille=pm,
                                                                 penalty=P, min_matched=m, boxes=True, matched=True, job_index=True, **kw),
                           args.reps)
            t["detections"] = int(len(out[0]))
            row[gate] = t
            print(f"windows gate {gate}: {t}", flush=True)
        res["windows"] = row
    return res


def compare(args):
    """The parent's build and this one as processes in turn, --rounds times each."""
    runs = []
    for r in range(args.rounds):
        for who, root in (("parent", args.parent), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", root, "--reps", str(args.reps), "--strides", args.strides,
                   "--min-matched", str(args.min_matched), "--line-caps", str(args.line_caps), "--overlap", str(args.overlap),
                   "--tau", str(args.tau)] + (["--skip-windows"] if args.skip_windows else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
            if out.returncode != 0:
                raise SystemExit(f"{who} (round {r}) failed:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
            res = json.loads(out.stdout.strip().splitlines()[-1])
            res["build"], res["round"] = who, r
            runs.append(res)
            print(f"round {r}: {who} done", flush=True)
    return {"workload": "config 2': 1024x1024 scene (200 lines, seed 1), depth 30, L2, padding 1.0; dense: 1000 templates x 32 lines "
                        "(seed 2), default window per stride, ExponentialPenalty(%g), max_detections 64; windows: 100 templates, 800 "
                        "seeds, 11 x 9 x 9 poses of 360 angles, DefaultPenalty, max_detections 1024" % args.tau, "runs": runs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--strides", default="1,2,4")
    ap.add_argument("--tau", type=float, default=1.5)
    ap.add_argument("--line-caps", type=float, default=3.0)
    ap.add_argument("--min-matched", type=float, default=0.26)
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
