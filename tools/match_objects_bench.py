"""Times the match lists with objects and hull shapes (include/fdcm.h, "Match lists: objects and hull shapes") on one GPU, on the
records of one config-2' frame as tools/match_detect_bench.py sets it up (1024 x 1024, 200 scene lines, 1000 templates of 32
lines, DefaultSearch(4, 4), BatchOptimize(10): about 27 000 records), DefaultPenalty, overlap 0.3, cross overlap 0.8,
max_detections 64, rescore off, host records:

  detect_matches          the call both builds have (the yardstick: this build's figure is read against the parent's two
                          processes, the machine code being the same)
  objects box / hull      detect_matches_objects at G = 1, 4 and 16 (objects t % G) on a BOX and on a HULL list
  shapes                  match_shapes of all records: the scan, k_matches_shapes and the table's download
  composition (hull)      what a caller had before, for the HULL list at each G: match_footprint_spans on the host and the rule in
                          numpy on its table (the candidates by verify_matches and penalize); the tool fails unless it returns
                          the same records

Each figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.  One process measures
one build (--package-root).  With --parent DIR the tool runs itself as processes in turn, the build under DIR and this one,
--rounds times each, and writes all of it to --json.  --trace makes one call of each kind and nothing else: the run for
rocprofv3 --kernel-trace --stats, a run of its own, whose kernel_stats.csv --kernel-stats puts into the JSON.

    python tools/match_objects_bench.py [--reps 5] [--package-root DIR] [--json out.json]
    python tools/match_objects_bench.py --parent DIR [--rounds 2] --json profiles/match_objects_bench_config2p.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = dict(overlap=0.3, max_detections=64)
CROSS = 0.8
GS = (1, 4, 16)


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def composition(openfdcm, fm, tmpls, matches, objects):
    """(records, positions) of detect_matches_objects on the hull list by the calls that existed before it and the host's span
    table: the rule on shapes in numpy, int64."""
    rec = matches.records()
    n = len(rec)
    q = openfdcm.penalize(openfdcm.DefaultPenalty(), matches, openfdcm.get_template_lengths(tmpls)).records()["score"]
    s = openfdcm.verify_matches(fm, tmpls, matches)[0]
    ok = ~np.isnan(s) & ~np.isnan(q) & ~np.signbit(q)
    off, spans, areas = openfdcm.match_footprint_spans(tmpls, matches)
    boxes = openfdcm.match_footprints(tmpls, matches).astype(np.int64)
    obj = np.asarray(objects)[rec["tmpl_idx"]]
    keys = (q.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    order = [int(j) for j in np.argsort(keys, kind="stable") if ok[j]]
    alive = np.zeros(n, dtype=bool)
    alive[order] = True
    pm, cr = int(round(1000 * RULE["overlap"])), int(round(1000 * CROSS))
    out = []
    for d in order:
        if len(out) == RULE["max_detections"]:
            break
        if not alive[d]:
            continue
        out.append(d)
        alive[d] = False
        cand = np.flatnonzero(alive & (boxes[:, 0] <= boxes[d, 2]) & (boxes[:, 2] >= boxes[d, 0]) & (boxes[:, 1] <= boxes[d, 3]) & (boxes[:, 3] >= boxes[d, 1]))
        for e in cand:
            ya, yb = max(boxes[d, 1], boxes[e, 1]), min(boxes[d, 3], boxes[e, 3])
            a = spans[off[d] + ya - boxes[d, 1]:off[d] + yb - boxes[d, 1] + 1].astype(np.int64)
            b = spans[off[e] + ya - boxes[e, 1]:off[e] + yb - boxes[e, 1] + 1].astype(np.int64)
            w = np.minimum(a[:, 1] + boxes[d, 0], b[:, 1] + boxes[e, 0]) - np.maximum(a[:, 0] + boxes[d, 0], b[:, 0] + boxes[e, 0]) + 1
            inter = int(np.maximum(0, w).sum())
            if 1000 * inter > (pm if obj[e] == obj[d] else cr) * (int(areas[d]) + int(areas[e]) - inter):
                alive[e] = False
    idx = np.array(out, dtype=np.int32)
    res = np.array(rec[idx])
    res["score"] = q[idx]
    return res, idx


def measure(args):
    sys.path.insert(0, os.path.abspath(args.package_root))
    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic

    has = hasattr(openfdcm, "detect_matches_objects")
    cfg, scene, tmpls = synthetic.make_config("2p")
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0, padding=1.0, distance=openfdcm.distance(cfg["distance"]))
    fm = openfdcm.build_cpu_featuremap(scene, params)
    matches = openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(4, 4), openfdcm.BatchOptimize(10), fm, tmpls, scene)
    pen = openfdcm.DefaultPenalty()
    res = {"package": os.path.relpath(os.path.abspath(args.package_root), ROOT), "has_objects": has, "records": len(matches)}
    calls = {"detect_matches": lambda: openfdcm.detect_matches(fm, tmpls, matches, penalty=pen, return_indices=True, **RULE)}
    if has:
        hull = openfdcm.with_footprint(tmpls, "hull")
        for G in GS:
            objects = np.arange(len(tmpls), dtype=np.int32) % G
            for name, lst in (("box", tmpls), ("hull", hull)):
                calls[f"objects_{name}_G{G}"] = (lambda lst=lst, objects=objects: openfdcm.detect_matches_objects(
                    fm, lst, matches, objects, cross_overlap=CROSS, penalty=pen, return_indices=True, **RULE))
        calls["shapes"] = lambda: openfdcm.match_shapes(fm, tmpls, matches)
    if args.trace:
        for name, call in calls.items():
            out = call()
            print(name, len(out[0]), flush=True)
        return res
    outs = {}
    for name, call in calls.items():
        outs[name], res[name] = timed(call, args.reps)
        res[name]["returned"] = int(len(outs[name][0])) if name != "shapes" else int(outs[name][0][-1])
        print(name, res[name], flush=True)
    if has:
        same = True
        for G in GS:
            t0 = time.perf_counter()
            want = composition(openfdcm, fm, tmpls, matches, np.arange(len(tmpls), dtype=np.int32) % G)
            res[f"composition_hull_G{G}"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "runs": 1}
            got = outs[f"objects_hull_G{G}"]
            same &= got[0].records().tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
        res["identical_to_composition"] = bool(same)
        res["box_and_hull_differ"] = bool(outs["objects_box_G1"][0].records().tobytes() != outs["objects_hull_G1"][0].records().tobytes())
        res["G1_box_is_detect_matches"] = bool(outs["objects_box_G1"][0].records().tobytes() == outs["detect_matches"][0].records().tobytes())
        if not same:
            print(json.dumps(res))
            sys.exit("the call and the composition of the calls before it differ")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", default=None, help="the parent commit's checkout, built: processes of both builds in turn")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.parent is None:
        res = measure(args)
        print("RESULT " + json.dumps(res), flush=True)
        if args.json and not args.trace:
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
            print(runs[-1]["package"], runs[-1]["detect_matches"], flush=True)
    res = {"workload": "the records of one config-2' frame (1024 x 1024, 200 scene lines, 1000 templates of 32 lines, DefaultSearch(4, 4), "
                       "BatchOptimize(10)); DefaultPenalty, overlap 0.3, cross overlap 0.8, max_detections 64, rescore off, host records",
           "protocol": f"median of {args.reps} blocking calls after a warm-up; processes in turn, the parent's build and this one, {args.rounds} each",
           "runs": runs,
           "not_measured": ["lists above one frame's records", "more than one batch of rounds (max_detections above 64)", "margins above 0",
                            "templates above 32 lines", "line caps and the gate", "HBM traffic and counters (no --pmc run)",
                            "the host-libm path", "the cost of the 64-bit divisions on their own", "more than one GPU"]}
    if args.kernel_stats:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from coverage_bench import kernel_split
        res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/match_objects_bench.py --trace, a run of its own: after "
                                         "the set-up (the build, one search) one call of each kind",
                               "kernels": [k for k in kernel_split(args.kernel_stats)
                                           if any(w in k["kernel"] for w in ("matches", "nms_round", "shape_rows"))]}
    else:
        res["not_measured"].append("the kernels' own times (no --kernel-stats file given)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_trace"}))


if __name__ == "__main__":
    main()
