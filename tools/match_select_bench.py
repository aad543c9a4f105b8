"""Scene coverage and selection of match records (include/fdcm.h, "Match lists: scene coverage and selection") on the records of
one search(): what the calls cost, against what a caller had before them.

The frame is tools/select_bench.py's: the config-2' scene rendered into a 1024 x 1024 frame, its edge labels and the map built
from it; 100 templates x 32 lines; the records are those of one search() on that map.  Timed: match_coverage on all records,
select_matches on the 64 and the 1024 best after detect_matches(overlap=1.0); host records and device records (the last
search's, and the labels on the device); median of --reps blocking calls after a warm-up.  Compared against the referee on the
host, once (tests/match_coverage_ref.py; for the coverage on the first --referee records, since it keeps an image per
record), and for the selection against one match_coverage call per candidate on the running residual.  The tool fails unless
all return the same bytes.

    python tools/match_select_bench.py [--reps 5] [--json profiles/match_select_bench_config2p.json]
    python tools/match_select_bench.py --trace      one call of each kind and nothing else: the run to trace"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARAMS = dict(radius=2, bin_tolerance=1)
RULE = dict(min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024)


def composition(openfdcm, fm, labels, tmpls, recs):
    """One match_coverage call per candidate on the running residual: (selected, counts (k, 3), residual tensor)."""
    counts = openfdcm.match_coverage(fm, labels, tmpls, recs, **PARAMS)
    share, pix = int(round(1000 * RULE["min_new"])), RULE["min_pixels"]
    running, sel, rows = labels, [], []
    for q in range(len(recs)):
        edges, explained = int(counts[q, 0]), int(counts[q, 1])
        if len(sel) == RULE["max_selected"]:
            break
        if explained < pix:
            continue
        c, r = openfdcm.match_coverage(fm, running, tmpls, recs[q:q + 1], return_residual=True, **PARAMS)
        new = int(c[0, 1])
        if new >= pix and 1000 * new >= share * explained:
            running = r
            sel.append(q)
            rows.append((edges, explained, new))
    return np.asarray(sel, dtype=np.int32), np.asarray(rows, dtype=np.int32).reshape(-1, 3), running


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--templates", type=int, default=100)
    ap.add_argument("--referee", type=int, default=256)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic
    from pyramid_bench import EDGE, RENDERING, render, timed
    import match_coverage_ref as MC

    cfg, scene, tmpls = synthetic.make_config("2p")
    frame = render(scene)
    sub = tmpls[: args.templates]
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0)
    labels = openfdcm.edge_labels(frame, depth=cfg["depth"], **EDGE)
    fm = openfdcm.build_image_featuremap(frame, params, **EDGE)
    dm = openfdcm._device_map(fm)
    m = len(dm.keys)
    t_lab = torch.from_numpy(labels).cuda()

    def search():
        return openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(4, 4), openfdcm.BatchOptimize(10), fm, sub, scene)
    matches = search()
    recs = matches.records()
    if args.trace:
        c = openfdcm.match_coverage(fm, t_lab, sub, None, **PARAMS)
        print("coverage", len(c), flush=True)
        for n in (64, 1024):
            best = openfdcm.detect_matches(fm, sub, matches, overlap=1.0, penalty=openfdcm.DefaultPenalty(), max_detections=n)
            sel, counts = openfdcm.select_matches(fm, t_lab, sub, best, **PARAMS, **RULE)
            print(n, "selected", len(sel), flush=True)
        return
    res = {"workload": "config 2' scene rendered into a 1024 x 1024 frame, labels of edge_labels, the records of one search() on the frame's map",
           "rendering": RENDERING, "edge": EDGE, "templates": len(sub), "lines_per_template": int(np.asarray(sub[0]).reshape(4, -1).shape[1]),
           "records": int(len(recs)), "edge_pixels": int((labels < m).sum()), "slices": m,
           "parameters": dict(PARAMS, margin=PARAMS["radius"], **RULE),
           "protocol": f"median of {args.reps} blocking calls after a warm-up, smallest and largest beside it; the referee once", "cases": []}
    # ---- match_coverage on all records
    case = {"call": "match_coverage", "records": int(len(recs))}
    (c1, r1), case["host_records"] = timed(lambda: openfdcm.match_coverage(fm, labels, sub, recs, return_residual=True, **PARAMS), args.reps)
    (c2, r2), case["last_search_device_labels"] = timed(lambda: openfdcm.match_coverage(fm, t_lab, sub, None, return_residual=True, **PARAMS), args.reps)
    same = np.array_equal(c1, c2) and np.array_equal(r1, r2.cpu().numpy())
    k = min(args.referee, len(recs))
    t0 = time.perf_counter()
    want = MC.coverage(labels, dm.keys, dm.scene_translation, dm.width, dm.height, sub, recs[:k], margin=PARAMS["radius"], **PARAMS)
    case["referee_host"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1, "records": int(k)}
    ck, rk = openfdcm.match_coverage(fm, labels, sub, recs[:k], return_residual=True, **PARAMS)
    same = same and np.array_equal(ck, want[0]) and np.array_equal(rk, want[1]) and np.array_equal(c1[:k], want[0])
    case["admissible"] = int((c1[:, 0] >= 0).sum())
    case["identical"] = bool(same)
    res["cases"].append(case)
    print("coverage", {k2: round(v["median_ms"], 3) for k2, v in case.items() if isinstance(v, dict) and "median_ms" in v}, flush=True)
    if not same:
        sys.exit("match_coverage: the forms or the referee differ")
    # ---- select_matches on the 64 and 1024 best
    for n in (64, 1024):
        best = openfdcm.detect_matches(fm, sub, matches, overlap=1.0, penalty=openfdcm.DefaultPenalty(), max_detections=n)
        brec = best.records()
        buf = torch.from_numpy(np.frombuffer(brec.tobytes(), dtype=np.uint8).copy()).cuda()
        case = {"call": "select_matches", "candidates": int(len(brec))}
        (sel, counts, resid), case["host_records"] = timed(
            lambda: openfdcm.select_matches(fm, labels, sub, brec, return_residual=True, **PARAMS, **RULE), args.reps)
        (s2, c2, r2), case["device_records_device_labels"] = timed(
            lambda: openfdcm.select_matches(fm, t_lab, sub, None, return_residual=True, device_ptr=buf.data_ptr(), n=len(brec), **PARAMS, **RULE),
            args.reps)
        (s3, c3, r3), case["composition"] = timed(lambda: composition(openfdcm, fm, t_lab, sub, brec), max(1, args.reps // 2))
        same = (np.array_equal(sel, s2) and np.array_equal(counts, c2) and np.array_equal(resid, r2.cpu().numpy())
                and np.array_equal(sel, s3) and np.array_equal(counts, c3) and np.array_equal(resid, r3.cpu().numpy()))
        if n == 64:
            t0 = time.perf_counter()
            want = MC.select(labels, dm.keys, dm.scene_translation, dm.width, dm.height, sub, brec, margin=PARAMS["radius"], **PARAMS, **RULE)
            case["referee_host"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
            same = same and np.array_equal(sel, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(resid, want[2])
        case["identical"] = bool(same)
        case["selected"] = int(len(sel))
        case["claimed_pixels"] = int((resid != labels).sum())
        case["speedup_over_composition"] = case["composition"]["median_ms"] / case["device_records_device_labels"]["median_ms"]
        res["cases"].append(case)
        print(n, "selected", len(sel), {k2: round(v["median_ms"], 3) for k2, v in case.items() if isinstance(v, dict) and "median_ms" in v},
              flush=True)
        if not same:
            sys.exit("select_matches: the forms, the composition or the referee differ")
    res["not_measured"] = ["HBM traffic and counters (no --pmc run)", "more than one GPU", "lists above one frame's records",
                           "the host-libm path's cost", "coverage in more than one part", "templates of more than 256 lines"]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
