"""Times the hull footprints (include/fdcm.h, "Hull footprints") against the box rule, on config 2' (bench.py's feature map and
its 1000 x 32-line synthetic templates), line caps 3, ExponentialPenalty(1.5), overlap 0.3:

  dense      per stride (1, 2, 4) on the default window, at max_score = +inf, max_detections 64 and 8:
               detect_all       exhaustive_detect_all on a set made the way every build makes it (the yardstick, and its spread)
               box, hull        the same call on a BOX and on a HULL set (builds that have the kinds); (t64 - t8) / 56 is the cost
                                of a round; span_host_ms is the host time of the span table alone (footprint_spans)
               composed         what was available before: best_score_map to the host and the greedy rule of tests/hull_ref.py
                                on its planes (--composed; stride 4 only: it is Python)
  rotations  100 templates x 36 angles, stride 4: the same three
  windows    tools/window_detect_bench.py's refinement workload (100 templates, 800 seeds, boxes of 11 x 9 x 9 poses on a table
             of 360 angles): exhaustive_detect_windows on a BOX and on a HULL set

Each figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.  One process measures
one build (--package-root).  With --parent DIR the tool runs itself as processes in turn, the build under DIR and this one,
--rounds times each, and writes all of it to --json: this build's BOX rows are read against the parent's detect_all and the
spread of the parent's own runs.

    python tools/hull_bench.py [--reps 5] [--strides 1,2,4] [--skip-windows] [--composed] [--package-root DIR] [--json out.json]
    python tools/hull_bench.py --parent DIR [--rounds 2] --json profiles/hull_bench_config2p.json
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
    import openfdcm_amd as openfdcm
    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates

    has = hasattr(DeviceTemplates, "footprint_spans")
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    pm = int(round(1000 * args.overlap))
    pen, tau = _capi.EXPONENTIAL_PENALTY, args.tau
    res = {"package": os.path.relpath(os.path.abspath(args.package_root), ROOT), "has_hull": has, "line_caps": args.line_caps,
           "overlap_permille": pm, "dense": [], "rotations": None, "windows": None}

    def sets(t):
        out = {"detect_all": DeviceTemplates(t, line_caps=args.line_caps)}
        if has:
            out["box"] = DeviceTemplates(t, line_caps=args.line_caps, footprint="box")
            out["hull"] = DeviceTemplates(t, line_caps=args.line_caps, footprint="hull")
        return out

    def dense(row, tsets, grid, cs=None, piv=None, p=pen):
        for name, tset in tsets.items():
            for md in (64, 8):
                out, t = timed(lambda: dev.exhaustive_detect_all(tset, grid, cs, piv, max_detections=md, overlap_permille=pm, penalty=p, tau=tau,
                                                                 boxes=True), args.reps)
                t["detections"] = int(len(out[0]))
                row[f"{name}_{md}"] = t
            row[f"{name}_us_per_round"] = round((row[f"{name}_64"]["median_ms"] - row[f"{name}_8"]["median_ms"]) / 56 * 1e3, 2)
            print(row.get("stride"), name, row[f"{name}_64"], row[f"{name}_8"], row[f"{name}_us_per_round"], flush=True)
        if has:
            _, t = timed(lambda: tsets["hull"].footprint_spans(cs, piv), args.reps)
            row["span_host_ms"] = t
            off = tsets["hull"].footprint_spans(cs, piv)[0]
            row["span_rows"] = int(off[-1])

    for s in [int(v) for v in args.strides.split(",") if v]:
        tsets = sets(tmpls)
        grid = dev.exhaustive_window(tsets["detect_all"], s, s).as_tuple()
        row = {"stride": s, "grid": list(grid), "grid_points": grid[2] * grid[3]}
        dense(row, tsets, grid)
        if args.composed and has and s == 4:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import hull_ref as hr
            shapes = hr.shapes(tmpls, margin=0)

            def composed():
                scores, pairs = dev.best_map(tsets["detect_all"], grid, penalty=pen, tau=tau)
                return hr.hull_objects_nms(scores, pairs, shapes, grid, 64, pm)
            out, t = timed(composed, 1)
            t["detections"] = int(len(out))
            row["composed_64"] = t
            print(s, "composed", t, flush=True)
        res["dense"].append(row)

    sub = tmpls[:100]
    piv = openfdcm.template_pivots(sub)
    coarse, fine = np.arange(36) * (2 * np.pi / 36), np.arange(360) * (2 * np.pi / 360)
    ccs, fcs = openfdcm._angles(coarse), openfdcm._angles(fine)
    wsets = sets(sub)
    grid = dev.exhaustive_rotations_window(wsets["detect_all"], ccs, piv, 4, 4).as_tuple()
    row = {"stride": 4, "templates": 100, "angles": 36, "grid": list(grid)}
    dense(row, wsets, grid, ccs, piv, _capi.DEFAULT_PENALTY)
    res["rotations"] = row

    if not args.skip_windows:
        P = _capi.DEFAULT_PENALTY
        seeds = dev.exhaustive_detect_all(wsets["detect_all"], grid, ccs, piv, max_detections=800, overlap_permille=1000, penalty=P)
        jobs = openfdcm.pose_windows(seeds, coarse, fine, piv, 5, 4, 4, wrap=True)
        row = {"jobs": int(len(jobs)), "box": [int(jobs[0, 2]), int(jobs[0, 5]), int(jobs[0, 6])]}
        for name, tset in wsets.items():
            out, t = timed(lambda: dev.exhaustive_detect_windows(tset, jobs, fcs, piv, wrap=True, max_detections=1024, overlap_permille=pm,
                                                                 penalty=P, boxes=True, job_index=True), args.reps)
            t["detections"] = int(len(out[0]))
            row[name] = t
            print("windows", name, t, flush=True)
        res["windows"] = row
    return res


def compare(args):
    """The parent's build and this one as processes in turn, --rounds times each."""
    runs = []
    for r in range(args.rounds):
        for who, root in (("parent", args.parent), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", root, "--reps", str(args.reps), "--strides", args.strides,
                   "--line-caps", str(args.line_caps), "--overlap", str(args.overlap), "--tau", str(args.tau)]
            cmd += (["--skip-windows"] if args.skip_windows else []) + (["--composed"] if args.composed and who == "this" and r == 0 else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit(f"{who} (round {r}) failed:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
            res = json.loads(out.stdout.strip().splitlines()[-1])
            res["build"], res["round"] = who, r
            runs.append(res)
            print(f"round {r}: {who} done", flush=True)
    return {"workload": "config 2': 1024x1024 scene (200 lines, seed 1), depth 30, L2, padding 1.0; dense: 1000 templates x 32 lines "
                        "(seed 2), default window per stride, ExponentialPenalty(%g), max_detections 64 and 8; rotations: 100 templates x "
                        "36 angles at stride 4, DefaultPenalty; windows: 100 templates, 800 seeds, 11 x 9 x 9 poses of 360 angles, "
                        "DefaultPenalty, max_detections 1024" % args.tau,
            "runs": runs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--strides", default="1,2,4")
    ap.add_argument("--tau", type=float, default=1.5)
    ap.add_argument("--line-caps", type=float, default=3.0)
    ap.add_argument("--overlap", type=float, default=0.3)
    ap.add_argument("--skip-windows", action="store_true")
    ap.add_argument("--composed", action="store_true")
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
