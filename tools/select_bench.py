"""Times scene selection (include/fdcm.h, "Scene selection") on one GPU, on the workload of tools/coverage_bench.py: config 2'
rendered into a 1024 x 1024 frame, the labels of edge_labels, the first --templates templates of config 2' (32 lines each), and
the poses of 64 and of 1024 detections of exhaustive_detect_all (max_score inf, overlap 1.0: the N best poses, best first, which
cluster, so most candidates conflict with an accepted one).  radius 2, bin_tolerance 1, margin = radius, min_new 0.5, the other
parameters at their defaults.

  scene_select             host labels in, host residual out
  scene_select_device      the labels a CUDA tensor, the residual staying on the device
  composition              what the caller could write before this call (include/fdcm.h, identity 8): one scene_coverage call on
                           the labels for the static test, then one per candidate on the running residual, a CUDA tensor
  referee_host             tests/select_ref.py on the host for the 64 poses, once

Each device figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest.  The call, the
composition and (for the 64 poses) the referee must select the same poses with the same counts and residual, or the tool
fails.  With --kernel-stats CSV (the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool with --trace, a run of
its own, which makes one call per list and nothing else after the set-up) the launches per call go into the JSON as well.

    python tools/select_bench.py [--reps 5] [--json profiles/select_bench_config2p.json]
"""
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


def composition(openfdcm, fm, labels, tmpls, poses):
    """Identity 8 on the device: (selected, counts (k, 3), residual tensor)."""
    counts = openfdcm.scene_coverage(fm, labels, tmpls, poses, **PARAMS)
    share, pix = int(round(1000 * RULE["min_new"])), RULE["min_pixels"]
    running, sel, rows = labels, [], []
    for q in range(len(poses)):
        edges, explained = int(counts[q, 0]), int(counts[q, 1])
        if len(sel) == RULE["max_selected"]:
            break
        if explained < pix:            # (min_coverage is 0: every admissible pose with a pixel is a candidate)
            continue
        c, r = openfdcm.scene_coverage(fm, running, tmpls, poses[q:q + 1], return_residual=True, **PARAMS)
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
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--trace", action="store_true", help="one scene_select call per list and nothing else: the run to trace")
    args = ap.parse_args()
    import torch
    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic
    from coverage_bench import kernel_split
    from pyramid_bench import EDGE, RENDERING, render, timed

    cfg, scene, tmpls = synthetic.make_config("2p")
    frame = render(scene)
    sub = tmpls[: args.templates]
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0)
    labels = openfdcm.edge_labels(frame, depth=cfg["depth"], **EDGE)
    fm = openfdcm.build_image_featuremap(frame, params, **EDGE)
    dm = openfdcm._device_map(fm)
    m = len(dm.keys)
    t_lab = torch.from_numpy(labels).cuda()
    res = {"workload": "config 2' scene rendered into a 1024 x 1024 frame, labels of edge_labels, scene selection over detections, best first",
           "rendering": RENDERING, "edge": EDGE, "templates": len(sub), "lines_per_template": int(np.asarray(sub[0]).reshape(4, -1).shape[1]),
           "edge_pixels": int((labels < m).sum()), "slices": m, "parameters": dict(PARAMS, margin=PARAMS["radius"], **RULE),
           "protocol": f"median of {args.reps} blocking calls after a warm-up, smallest and largest beside it; the referee once",
           "cases": []}
    for n in (64, 1024):
        dets = openfdcm.exhaustive_detect_all(fm, sub, float("inf"), overlap=1.0, max_detections=n, penalty=openfdcm.DefaultPenalty())
        poses = openfdcm.record_poses(dets)
        if args.trace:
            sel, counts = openfdcm.scene_select(fm, t_lab, sub, poses, **PARAMS, **RULE)
            print(n, "selected", len(sel), flush=True)
            continue
        case = {"candidates": int(len(poses))}
        (sel, counts, resid), case["scene_select"] = timed(
            lambda: openfdcm.scene_select(fm, labels, sub, poses, return_residual=True, **PARAMS, **RULE), args.reps)
        (s2, c2, r2), case["scene_select_device"] = timed(
            lambda: openfdcm.scene_select(fm, t_lab, sub, poses, return_residual=True, **PARAMS, **RULE), args.reps)
        (s3, c3, r3), case["composition"] = timed(lambda: composition(openfdcm, fm, t_lab, sub, poses), args.reps)
        same = (np.array_equal(sel, s2) and np.array_equal(counts, c2) and np.array_equal(resid, r2.cpu().numpy())
                and np.array_equal(sel, s3) and np.array_equal(counts, c3) and np.array_equal(resid, r3.cpu().numpy()))
        case["identical_to_composition"] = bool(same)
        case["selected"] = int(len(sel))
        case["claimed_pixels"] = int((resid != labels).sum())
        case["speedup_over_composition"] = case["composition"]["median_ms"] / case["scene_select_device"]["median_ms"]
        if not same:
            sys.exit("the call and the composition of scene_coverage calls differ")
        if n == 64:
            import select_ref
            t0 = time.perf_counter()
            want = select_ref.select(labels, dm.keys, dm.scene_translation, dm.width, dm.height, sub, poses, margin=PARAMS["radius"],
                                     **PARAMS, **RULE)
            case["referee_host"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
            case["identical_to_referee"] = bool(np.array_equal(sel, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(resid, want[2]))
            if not case["identical_to_referee"]:
                sys.exit("the device's selection differs from the referee's")
        res["cases"].append(case)
        print(n, "selected", len(sel), {k: round(v["median_ms"], 3) for k, v in case.items() if isinstance(v, dict) and "median_ms" in v},
              flush=True)
    if args.trace:
        return
    res["not_measured"] = ["HBM traffic and counters (no --pmc run)", "more than one GPU", "poses with rotations", "label images from a camera",
                           "templates of more than 256 lines", "lists of more than 1024 candidates"]
    if args.kernel_stats:
        res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/select_bench.py --trace, a run of its own: after "
                                         "the set-up (edge labels, the map, two exhaustive_detect_all calls) one scene_select call on the 64 "
                                         "and one on the 1024 poses, labels on the device, no residual",
                               "kernels": [k for k in kernel_split(args.kernel_stats) if "select" in k["kernel"] or "coverage" in k["kernel"]]}
    else:
        res["not_measured"].append("the launches per call (no --kernel-stats file given)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_trace"}))


if __name__ == "__main__":
    main()
