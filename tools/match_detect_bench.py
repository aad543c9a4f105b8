"""Times the calls on match lists (include/fdcm.h, "Match lists") on one GPU, on the records of one config-2' frame (1024 x 1024,
200 scene lines, 1000 templates of 32 lines, DefaultSearch(4, 4), BatchOptimize(10): about 27 000 records): detect_matches
with DefaultPenalty, overlap 0.3 and max_detections 64, without caps and with line_caps = 3 and min_matched = 0.1, the score
the record's own (rescore off).

  host           the records a MatchList on the host (uploaded by the call)
  device         the records in a device buffer filled by search_into
  last_search    the records the handle kept from the last search()
  composition    what a caller of search() had before these calls, in the same process: penalize and a stable order by
                 (score, position), the posed lines in numpy float32, fdcm_featuremap_evaluate on the posed templates for
                 admissibility and (with caps) on one-line templates for the line costs, the matched length, the boxes and
                 the greedy rule in numpy

The public call's own Python work is inside every device figure: with a scalar line_caps the template cache recomputes the
32 000 caps from the template list on every call, about 2 ms.

Each device figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.  The tool fails
unless all forms and the composition return the same records, positions and boxes.  Also reported, not asserted: the share
of records whose s(r) has the bits of the search's score, and the share that is admissible.  With --kernel-stats CSV (the
kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool with --trace, a run of its own, which after the set-up
makes one call per input form and variant and nothing else) the launches and kernel times go into the JSON as well.

    python tools/match_detect_bench.py [--reps 5] [--json profiles/match_detect_bench_config2p.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
RULE = dict(overlap=0.3, max_detections=64)
CAPPED = dict(line_caps=3.0, min_matched=0.1)


def posed_lines(tmpls, rec):
    """(n, 4, L) float32 posed lines of records whose templates all have L lines: transform, math.h:341-344, unfused."""
    T = np.stack([np.asarray(t, dtype=np.float32) for t in tmpls])[rec["tmpl_idx"]]      # (n, 4, L)
    M = rec["transform"]
    out = np.empty_like(T)
    for r in (0, 2):
        out[:, r] = (M[:, 0, None] * T[:, r] + M[:, 1, None] * T[:, r + 1]) + M[:, 2, None]
        out[:, r + 1] = (M[:, 3, None] * T[:, r] + M[:, 4, None] * T[:, r + 1]) + M[:, 5, None]
    return out


def composition(openfdcm, fm, tmpls, matches, capped):
    """(records, positions, boxes) of detect_matches by the calls that existed before it."""
    from window_detect_bench import list_nms
    dm = openfdcm._device_map(fm)
    rec = matches.records()
    n = len(rec)
    pen = openfdcm.penalize(openfdcm.DefaultPenalty(), matches, openfdcm.get_template_lengths(tmpls)).records()
    q = pen["score"]
    P = posed_lines(tmpls, rec)
    zero = np.zeros((1, 2), dtype=np.float32)
    score = np.array([s[0] for s in dm.evaluate(list(P), [zero] * n)], dtype=np.float32)      # NaN: not admissible
    ok = ~np.isnan(score) & ~np.isnan(q) & ~np.signbit(q)
    if capped:
        L = P.shape[2]
        caps = np.stack(openfdcm.line_caps(tmpls, CAPPED["line_caps"]))[rec["tmpl_idx"]]     # (n, L)
        lens = np.stack(openfdcm._engine.line_lengths(tmpls))[rec["tmpl_idx"]]
        rows = np.flatnonzero(ok)
        one = [P[j][:, i:i + 1] for j in rows for i in range(L)]
        cost = np.full((n, L), np.nan, dtype=np.float32)
        cost[rows] = np.array([s[0] for s in dm.evaluate(one, [zero] * len(one))], dtype=np.float32).reshape(len(rows), L)
        ml = np.zeros(n, dtype=np.float32)
        tl = np.zeros(n, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            for i in range(L):                                                                # sequential in line order, from +0
                ml = np.where(cost[:, i] <= caps[:, i], ml + lens[:, i], ml).astype(np.float32)
                tl = (tl + lens[:, i]).astype(np.float32)
        ok &= ml >= np.float32(CAPPED["min_matched"]) * tl
    xs, ys = P[:, [0, 2]].reshape(n, -1), P[:, [1, 3]].reshape(n, -1)
    with np.errstate(invalid="ignore"):
        boxes = np.stack([np.floor(xs.min(axis=1)), np.floor(ys.min(axis=1)), np.floor(xs.max(axis=1)), np.floor(ys.max(axis=1))], axis=1)
    boxes = np.where(ok[:, None], boxes, 0).astype(np.int64)
    keys = (q.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    keys[~ok] = np.uint64(2 ** 64 - 1)
    idx = list_nms(keys, boxes, int(round(1000 * RULE["overlap"])), RULE["max_detections"])
    return pen[idx], idx.astype(np.int32), boxes[idx].astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--trace", action="store_true", help="one call per input form and variant and nothing else: the run to trace")
    args = ap.parse_args()
    import torch
    import openfdcm_amd as openfdcm
    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import search_into
    from coverage_bench import kernel_split
    from hull_bench import timed

    cfg, scene, tmpls = synthetic.make_config("2p")
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0, padding=1.0, distance=openfdcm.distance(cfg["distance"]))
    fm = openfdcm.build_cpu_featuremap(scene, params)
    dm = openfdcm._device_map(fm)
    search = lambda: openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(4, 4), openfdcm.BatchOptimize(10), fm, tmpls, scene)  # noqa: E731
    matches = search()
    n = len(matches)
    tset = openfdcm._template_cache.get(tmpls)
    buf = torch.empty(tset.capacity(scene.shape[1], 4, 4) * 32, dtype=torch.uint8, device="cuda")
    assert search_into(dm, tset, scene, 4, 4, _capi.BATCH_OPTIMIZE, 10, 0, buf.data_ptr()) == n
    search()                                                                                  # the last search on the handle is the host-output one
    pen = openfdcm.DefaultPenalty()
    res = {"workload": "the records of one config-2' frame (1024 x 1024, 200 scene lines, 1000 templates of 32 lines, DefaultSearch(4, 4), "
                       "BatchOptimize(10)); detect_matches with DefaultPenalty, rescore off",
           "records": n, "parameters": dict(RULE, capped=CAPPED),
           "protocol": f"median of {args.reps} blocking calls after a warm-up, smallest and largest beside it", "cases": []}
    for capped in (False, True):
        kw = dict(RULE, penalty=pen, return_indices=True, return_boxes=True, **(CAPPED if capped else {}))
        forms = {"host": lambda: openfdcm.detect_matches(fm, tmpls, matches, **kw),
                 "device": lambda: openfdcm.detect_matches(fm, tmpls, None, device_ptr=buf.data_ptr(), n=n, **kw),
                 "last_search": lambda: openfdcm.detect_matches(fm, tmpls, None, **kw)}
        if args.trace:
            for name, call in forms.items():
                print(name, capped, len(call()[0]), flush=True)
            continue
        case = {"capped": capped}
        outs = {}
        for name, call in forms.items():
            outs[name], case[name] = timed(call, args.reps)
        t0 = time.perf_counter()
        want = composition(openfdcm, fm, tmpls, matches, capped)
        case["composition"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "runs": 1}
        same = all(o[0].records().tobytes() == want[0].tobytes() and np.array_equal(o[1], want[1]) and np.array_equal(o[2], want[2])
                   for o in outs.values())
        case["identical_to_composition"] = bool(same)
        case["returned"] = int(len(outs["host"][0]))
        s, f, _ = openfdcm.verify_matches(fm, tmpls, matches, line_caps=CAPPED["line_caps"] if capped else None)
        case["admissible_share"] = float((~np.isnan(s)).mean())
        case["matched_fraction_quantiles"] = {str(p): float(np.nanquantile(f, p)) for p in (0.5, 0.9, 0.99, 1.0)}
        case["s_equals_search_score_share"] = float((s.view(np.uint32) == matches.records()["score"].view(np.uint32)).mean())
        res["cases"].append(case)
        print(capped, {k: v.get("median_ms", v.get("ms")) for k, v in case.items() if isinstance(v, dict)}, "returned", case["returned"], flush=True)
        if not same:
            sys.exit("the call and the composition of the calls before it differ")
    if args.trace:
        return
    res["not_measured"] = ["lists above one frame's records", "more than one batch of rounds at this size (max_detections above 64)",
                           "HBM traffic and counters (no --pmc run)", "more than one GPU"]
    if args.kernel_stats:
        res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/match_detect_bench.py --trace, a run of its own: after "
                                         "the set-up (the build, three searches) one detect_matches call per input form, without and with caps",
                               "kernels": [k for k in kernel_split(args.kernel_stats) if "matches" in k["kernel"] or "nms_round" in k["kernel"]]}
    else:
        res["not_measured"].append("the launches per call (no --kernel-stats file given)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_trace"}))


if __name__ == "__main__":
    main()
