"""The pose fit of match records (include/fdcm.h, "Match lists: pose fit") on the records of one search(): what the call
costs, against the referee on the host.

The frame is tools/match_select_bench.py's: the config-2' scene rendered into a 1024 x 1024 frame, its edge labels and the map
built from it; 100 templates x 32 lines; the records are those of one search() on that map.  Timed: fit_matches at 1 and 2
iterations, on host records with host labels and on device records (the last search's) with the labels on the device; median
of --reps blocking calls after a warm-up.  Compared against the referee on the host, once, on the first --referee records
(tests/fit_ref.py).  The tool fails unless all return the same bytes.

Reported as well, asserted nowhere: the two-parts scene of tests/match_scene.py drawn into labels, and the largest distance
between a detected part's posed corners and the planted ones after search, search -> refine_matches and search ->
refine_matches -> fit_matches (each list through detect_matches with rescore).

    python tools/fit_bench.py [--reps 5] [--json profiles/fit_bench_config2p.json]
    python tools/fit_bench.py --trace      one call of each kind and nothing else: the run to trace"""
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
PARAMS = dict(radius=3, bin_tolerance=1)


def scene_errors(openfdcm):
    """The chain on match_scene's two parts: per stage the detected records' largest corner distance to the nearest planted pose."""
    import fit_cases as FC
    import match_scene as MS
    scene, tmpls, _ = MS.two_parts()
    depth, size = 30, 176
    import edge_ref
    from openfdcm_amd.engine import DeviceFeatureMap
    labels = np.full((size, size), 255, dtype=np.uint8)
    FC.draw(labels, scene.astype(np.float64), edge_ref.keys_of(depth))
    dev = openfdcm.Dt3Cpu(None, _device=DeviceFeatureMap.build_labels(labels, border=8, depth=depth))
    true = [np.array([np.cos(a), -np.sin(a), x, np.sin(a), np.cos(a), y]) for a, x, y in MS.POSES]
    searched = openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(MS.MAX_TMPL, MS.MAX_SCENE), openfdcm.BatchOptimize(10), dev,
                               tmpls, scene)
    refined = openfdcm.refine_matches(dev, tmpls, searched, angles=openfdcm.delta_angles(3, np.deg2rad(1.0)), half_x=3, half_y=3)
    fitted, info = openfdcm.fit_matches(dev, labels, tmpls, refined, return_info=True, **PARAMS)
    out = {"scene": "tests/match_scene.py: two instances of an eight-sided part and six clutter lines, drawn into %d x %d labels" % (size, size),
           "refine": "delta_angles(3, 1 degree), half_x = half_y = 3", "fit": dict(PARAMS, iterations=2),
           "fit_status": {str(k): int(v) for k, v in zip(*np.unique(info[:, 0], return_counts=True))}}
    for name, lst in (("search", searched), ("search_refine", refined), ("search_refine_fit", fitted)):
        kept = openfdcm.detect_matches(dev, tmpls, lst, max_score=MS.MAX_SCORE, overlap=0.3, penalty=openfdcm.DefaultPenalty(), rescore=True)
        errs = sorted(min(FC.error(r["transform"], t, MS.PART) for t in true) for r in kept.records())
        out[name] = {"detected": int(len(kept)), "corner_error_px": [round(float(e), 4) for e in errs]}
    return out


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
    import fit_ref as FR

    cfg, scene, tmpls = synthetic.make_config("2p")
    frame = render(scene)
    sub = tmpls[: args.templates]
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0)
    labels = openfdcm.edge_labels(frame, depth=cfg["depth"], **EDGE)
    fm = openfdcm.build_image_featuremap(frame, params, **EDGE)
    dm = openfdcm._device_map(fm)
    m = len(dm.keys)
    t_lab = torch.from_numpy(labels).cuda()
    matches = openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(4, 4), openfdcm.BatchOptimize(10), fm, sub, scene)
    recs = matches.records()
    if args.trace:
        for it in (1, 2):
            out = openfdcm.fit_matches(fm, t_lab, sub, None, iterations=it, **PARAMS)
            print("fit", it, len(out), flush=True)
        return
    res = {"workload": "config 2' scene rendered into a 1024 x 1024 frame, labels of edge_labels, the records of one search() on the frame's map",
           "rendering": RENDERING, "edge": EDGE, "templates": len(sub), "lines_per_template": int(np.asarray(sub[0]).reshape(4, -1).shape[1]),
           "records": int(len(recs)), "edge_pixels": int((labels < m).sum()), "slices": m,
           "parameters": dict(PARAMS, margin=PARAMS["radius"], min_pixels=8, damping=1e-3, max_shift=PARAMS["radius"], max_angle=0.1),
           "protocol": f"median of {args.reps} blocking calls after a warm-up, smallest and largest beside it; the referee once", "cases": []}
    k = min(args.referee, len(recs))
    for it in (1, 2):
        kw = dict(iterations=it, return_info=True, return_rms=True, **PARAMS)
        case = {"call": "fit_matches", "iterations": it, "records": int(len(recs))}
        (o1, i1, r1), case["host_records"] = timed(lambda: openfdcm.fit_matches(fm, labels, sub, recs, **kw), args.reps)
        (o2, i2, r2), case["last_search_device_labels"] = timed(lambda: openfdcm.fit_matches(fm, t_lab, sub, None, **kw), args.reps)
        same = o1.records().tobytes() == o2.records().tobytes() and i1.tobytes() == i2.tobytes() and r1.tobytes() == r2.tobytes()
        t0 = time.perf_counter()
        want = FR.fit(labels, dm.keys, dm.scene_translation, dm.width, dm.height, sub, recs[:k], iterations=it, **PARAMS)
        case["referee_host"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1, "records": int(k)}
        ok, ik, rk = openfdcm.fit_matches(fm, labels, sub, recs[:k], **kw)
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip((ok.records(), ik, rk), want))
        same = same and o1.records()[:k].tobytes() == want[0].tobytes() and i1[:k].tobytes() == want[1].tobytes()
        case["status"] = {str(s): int(c) for s, c in zip(*np.unique(i1[:, 0], return_counts=True))}
        case["fit_pixels_first_pass"] = int(i1[:, 2].sum())
        case["moved"] = int(np.any(o1.records()["transform"] != recs["transform"], axis=1).sum())
        case["identical"] = bool(same)
        res["cases"].append(case)
        print("fit", it, {k2: round(v["median_ms"], 3) for k2, v in case.items() if isinstance(v, dict) and "median_ms" in v}, case["status"],
              flush=True)
        if not same:
            sys.exit("fit_matches: the forms or the referee differ")
    res["two_parts_scene"] = scene_errors(openfdcm)
    print("two parts", res["two_parts_scene"], flush=True)
    res["not_measured"] = ["HBM traffic and counters (no --pmc run)", "more than one GPU", "lists above one frame's records",
                           "the host-libm path's cost", "a list in more than one part", "templates of more than 32 lines",
                           "records left on the device (out_device_ptr)"]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
