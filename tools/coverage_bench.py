"""Times scene coverage (include/fdcm.h, "Scene coverage") on one GPU: config 2' rendered into a 1024 x 1024 frame as
tools/pyramid_bench.py renders it, the labels of edge_labels, the first --templates templates of config 2' (32 lines each), and the
poses of 64 and of 1024 detections of exhaustive_detect_all (max_score inf, overlap 1.0: the N best poses, which cluster, so the
windows overlap -- the residual's many-writers case).  radius 2, bin_tolerance 1, margin = radius.

  scene_coverage           counts alone / counts and residual, host labels in and host residual out
  scene_coverage_device    the same with the labels a CUDA tensor and the residual staying on the device
  matched_fractions        the existing per-pose call of the same shape, on the same poses
  referee_host             tests/coverage_ref.py on the host for the 64 poses: the only way to these numbers without this call

Each device figure is the median of --reps blocking calls after a warm-up, with the smallest and the largest; the referee runs
once.  The device's counts and residual for the 64 poses must equal the referee's, or the tool fails.  With --kernel-stats CSV
(the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool, a run of its own) the kernels' split goes into
the JSON as well.

    python tools/coverage_bench.py [--reps 5] [--json profiles/coverage_bench_config2p.json]
"""
import argparse
import csv
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


def kernel_split(path):
    """Per kernel of a rocprofv3 kernel_stats.csv: calls, total and average nanoseconds, share."""
    out = []
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
            out.append({"kernel": name[5:] if name.startswith("void ") else name, "calls": int(row["Calls"]),
                        "total_ns": int(float(row["TotalDurationNs"])), "average_ns": float(row["AverageNs"]), "min_ns": int(float(row["MinNs"])),
                        "max_ns": int(float(row["MaxNs"])), "percent": float(row["Percentage"])})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--templates", type=int, default=100)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    try:
        import torch
    except Exception:  # the device-tensor figures are left out without it
        torch = None
    import openfdcm_amd as openfdcm
    from openfdcm_amd import synthetic
    from pyramid_bench import EDGE, RENDERING, render, timed

    cfg, scene, tmpls = synthetic.make_config("2p")
    frame = render(scene)
    sub = tmpls[: args.templates]
    params = openfdcm.Dt3CpuParameters(depth=cfg["depth"], dt3Coeff=5.0)
    labels = openfdcm.edge_labels(frame, depth=cfg["depth"], **EDGE)
    fm = openfdcm.build_image_featuremap(frame, params, **EDGE)
    m = len(fm._fm.keys)
    res = {"workload": "config 2' scene rendered into a 1024 x 1024 frame, labels of edge_labels, scene coverage of detections",
           "rendering": RENDERING, "edge": EDGE, "templates": len(sub), "lines_per_template": int(np.asarray(sub[0]).reshape(4, -1).shape[1]),
           "edge_pixels": int((labels < m).sum()), "slices": m, "parameters": dict(PARAMS, margin=PARAMS["radius"]),
           "protocol": f"median of {args.reps} blocking calls after a warm-up, smallest and largest beside it; the referee once",
           "cases": []}
    t_lab = torch.from_numpy(labels).cuda() if torch is not None else None
    for n in (64, 1024):
        dets = openfdcm.exhaustive_detect_all(fm, sub, float("inf"), overlap=1.0, max_detections=n, penalty=openfdcm.DefaultPenalty())
        poses = openfdcm.record_poses(dets)
        case = {"detections": int(len(poses))}
        counts, case["scene_coverage_counts"] = timed(lambda: openfdcm.scene_coverage(fm, labels, sub, poses, **PARAMS), args.reps)
        (c2, resid), case["scene_coverage_counts_and_residual"] = timed(
            lambda: openfdcm.scene_coverage(fm, labels, sub, poses, return_residual=True, **PARAMS), args.reps)
        assert np.array_equal(counts, c2)
        if t_lab is not None:
            c3, case["scene_coverage_device_counts"] = timed(lambda: openfdcm.scene_coverage(fm, t_lab, sub, poses, **PARAMS), args.reps)
            (c4, r4), case["scene_coverage_device_counts_and_residual"] = timed(
                lambda: openfdcm.scene_coverage(fm, t_lab, sub, poses, return_residual=True, **PARAMS), args.reps)
            assert np.array_equal(counts, c3) and np.array_equal(counts, c4) and np.array_equal(r4.cpu().numpy(), resid)
        _, case["matched_fractions"] = timed(lambda: openfdcm.matched_fractions(fm, sub, poses, line_caps=3.0), args.reps)
        adm = counts[:, 0] >= 0
        case["window_pixels_median"] = None
        case["edges_in_windows"] = {"min": int(counts[adm, 0].min()), "median": float(np.median(counts[adm, 0])), "max": int(counts[adm, 0].max())}
        case["explained_share"] = {"min": float((counts[adm, 1] / np.maximum(1, counts[adm, 0])).min()),
                                   "median": float(np.median(counts[adm, 1] / np.maximum(1, counts[adm, 0]))),
                                   "max": float((counts[adm, 1] / np.maximum(1, counts[adm, 0])).max())}
        case["residual_pixels_explained"] = int((resid != labels).sum())
        boxes = openfdcm.template_footprints(sub, margin=PARAMS["radius"])[poses[:, 0], 0].astype(np.int64)
        case["window_pixels_median"] = float(np.median((boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)))
        if n == 64:
            import coverage_ref
            t0 = time.perf_counter()
            want_c, want_r, _ = coverage_ref.coverage(labels, fm._fm.keys, fm._fm.scene_translation, fm._fm.width, fm._fm.height, sub, poses,
                                                      margin=PARAMS["radius"], **PARAMS)
            case["referee_host"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
            case["identical_to_referee"] = bool(np.array_equal(counts, want_c) and np.array_equal(resid, want_r))
            if not case["identical_to_referee"]:
                sys.exit("the device's counts or residual differ from the referee's")
        res["cases"].append(case)
        print(n, {k: round(v["median_ms"], 3) for k, v in case.items() if isinstance(v, dict) and "median_ms" in v}, flush=True)
    res["not_measured"] = ["HBM traffic and counters (no --pmc run)", "more than one GPU", "poses with rotations"]
    if args.kernel_stats:
        res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/coverage_bench.py, a run of its own",
                               "kernels": kernel_split(args.kernel_stats)}
    else:
        res["not_measured"].append("the kernel trace's split (no --kernel-stats file given)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_trace"}))


if __name__ == "__main__":
    main()
